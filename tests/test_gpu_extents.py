"""GPU: every reconstruction form at the widest and tallest pictures the library accepts (1 .. 1024 macroblocks each way,
params_ok in hotpath_abi.hip), planes and RGB byte for byte against oracle/recon_ref.c.

Picture width decides which form runs and with how many waves (every form keeps pictures x W x 32 bytes of line buffer in LDS:
as rows get longer the planner steps a form down through the wave counts it is built for and then hands over to a simpler
form), and it is a factor of every line-buffer, seam and strip offset; picture height is a factor of the pass, band, ticket and
seam counts.  tests/test_launch_plan.py pins the planner's decisions on the CPU; here the kernels those decisions lead to run:
* each forced form at every width at which mvhp_plan_launch changes its answer ON THIS DEVICE (the widths are scanned from the
  planner, not written down), at the width before it and at 1024, Baseline and High, plan == launch, and a census over what
  was really launched (test_census);
* the automatic choice at 1024, 1016, 1017, 860 and 477 macroblocks per row with 1, 9 and 600 pictures;
* every form at 255 .. 1023 columns (2^8 and 2^9 columns, 2^16-byte line offsets, widths 0, 1 and 3 modulo the strip), with
  unavailable-neighbour modes and QP 0 .. 51, and with the separate colour kernel on a row of 16 368 samples;
* every form at 1024, 1024, 1023 and 513 rows of 1, 2, 3 and 5 macroblocks, at every wave / row count it is built for;
* one context whose banded launches grow and shrink (3 x 1024, 1024 x 3, 20 x 17, 3 x 1024), and one 1024 x 64 picture.

The pictures of the width scans are the leftmost W columns of ONE synthetic picture 1024 macroblocks wide: synth_packed draws
each prediction mode from the availability of the left, upper and upper-left neighbours only, which the columns to the right do
not change, so the cropped picture is as legal as the whole one; the oracle runs on exactly the records the kernel gets."""
import functools
import time

import numpy as np
import pytest

from minivideo_amd import HotPath
from minivideo_amd.hotpath import LAYOUTS, PARAM_MAY_HAVE_8X8, StreamParams
from minivideo_amd.synth import synth_packed
from oracle import loader

pytestmark = pytest.mark.gpu

FORMS = LAYOUTS[1:]
PROFILES = ("baseline", "high")
# mvhp_set_waves_per_picture values each form is instantiated for (launch_plan.hip kernel_form(): waves per workgroup; banded
# forms: rows per band); "wide" has one
BUILT = {"rows": (4, 8, 16), "quad": (4, 6, 8, 12, 16), "oct": (4, 6, 8), "wide": (4,), "quad_wide": (4, 8), "pipe": (1, 2, 4),
         "pipe1": (1, 2, 4)}


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def ctx():
    """ctx(layout) -> this module's context with that layout set (one HotPath per form, made on first use)"""
    made = {}

    def get(layout):
        if layout not in made:
            made[layout] = HotPath(0)
            made[layout].set_layout(layout)
        return made[layout]

    yield get
    for h in made.values():
        h.close()


def _with_oracle(params, rec):
    return params, rec, [loader.recon(params, rec[k], 1, want_rgb=True) for k in range(rec.shape[0])]


@functools.lru_cache(maxsize=None)
def _source(profile, H, D):
    """D synthetic pictures of 1024 x H macroblocks as [D, H, 1024, 800]"""
    _, rec = synth_packed(1024, H, D, seed=31 * H + D + len(profile), profile=profile, density="dense")
    return rec.reshape(D, H, 1024, 800)


@functools.lru_cache(maxsize=4)
def _columns(W, H, profile, D):
    """the leftmost W columns of _source (module docstring): params, records [D, W * H, 800], the oracle's (planes, RGB) each"""
    rec = np.ascontiguousarray(_source(profile, H, D)[:, :, :W]).reshape(D, W * H, 800)
    return _with_oracle(StreamParams(W, H, 0, 0, PARAM_MAY_HAVE_8X8 if profile == "high" else 0), rec)


def _recon(torch, hot, params, rec, n, want_rgb=True):
    """n pictures tiled on the device from the distinct ones of rec; the plan asked for beforehand must be the launch.
    -> (layout, waves), planes [n, -1] and RGB [n, -1] (device)"""
    D = rec.shape[0]
    d_small = torch.from_numpy(rec.reshape(D, -1)).cuda()
    d_packed = d_small.repeat((n + D - 1) // D, 1)[:n].contiguous()
    d_yuv = torch.zeros(n * params.yuv_bytes, dtype=torch.uint8, device="cuda")
    d_rgb = torch.zeros(n * params.rgb_bytes, dtype=torch.uint8, device="cuda") if want_rgb else None
    torch.cuda.synchronize()
    plan = hot.plan_launch(params, n)
    hot.recon_dev(params, d_packed.data_ptr(), n, d_yuv.data_ptr(), d_rgb.data_ptr() if want_rgb else None, None)
    hot.sync_check(None)
    assert hot.last_launch() == plan, (hot.last_launch(), plan)
    return plan, d_yuv.view(n, -1), (d_rgb.view(n, -1) if want_rgb else None)


def _same(torch, got, ref, which, what):
    """every byte of got [n, -1] (device): picture f is ref[f % D][which]; compared on the device, a difference located on the host"""
    D = len(ref)
    for k in range(min(D, got.shape[0])):
        want = torch.from_numpy(np.ascontiguousarray(ref[k][which]).reshape(-1)).cuda()
        rows = got[k::D]
        bad = (rows != want).any(dim=1)
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            off = np.nonzero(rows[i].cpu().numpy() != ref[k][which].reshape(-1))[0]
            raise AssertionError("%s: picture %d: %d %s bytes differ from the oracle, first at offset %d" % (
                what, k + i * D, off.size, ("plane", "RGB")[which], int(off[0])))


def _run(torch, hot, params, rec, ref, n, what, want_rgb=True):
    got, yuv, rgb = _recon(torch, hot, params, rec, n, want_rgb)
    _same(torch, yuv, ref, 0, (what, got))
    if want_rgb:
        _same(torch, rgb, ref, 1, (what, got))
    return got


# ---- 1. each form at each width at which its plan changes ---------------------------------------------------------------------
STEP_H, STEP_N = 8, 9                  # 9 pictures: the four- and eight-picture forms get a short last group
_PLANNED, _LAUNCHED, _RAN = {}, {}, set()


def _plan_by_width(hot, flags):
    """what mvhp_plan_launch answers on this context for W = 1 .. 1024 (index W - 1)"""
    p = StreamParams(1, STEP_H, 0, 0, flags)
    out = []
    for W in range(1, 1025):
        p.width_mbs = W
        out.append(hot.plan_launch(p, STEP_N))
    return out


def _run_steps(torch, ctx, form, profile):
    hot = ctx(form)
    plans = _plan_by_width(hot, PARAM_MAY_HAVE_8X8 if profile == "high" else 0)
    steps = [W for W in range(2, 1025) if plans[W - 1] != plans[W - 2]]
    _PLANNED.setdefault(form, set()).update(plans)
    print("plan by width, %s, %s: %s" % (form, profile, [(1, plans[0])] + [(W, plans[W - 1]) for W in steps]))
    for W in sorted({1024} | set(steps) | {W - 1 for W in steps}):
        params, rec, ref = _columns(W, STEP_H, profile, 3)
        got = _run(torch, hot, params, rec, ref, STEP_N, (form, profile, W))
        assert got == plans[W - 1], (form, profile, W, got, plans[W - 1])
        _LAUNCHED.setdefault(form, set()).add(got)     # hot.last_launch() after a launch whose every byte was the oracle's
    _RAN.add((form, profile))


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("form", FORMS)
def test_every_width_at_which_the_plan_changes(torch_cuda, ctx, form, profile):
    _run_steps(torch_cuda, ctx, form, profile)
    torch_cuda.cuda.empty_cache()


def test_census(torch_cuda, ctx):
    """what the launches of the test above ran on (mvhp_last_launch_info after each), on the device at hand: every (form, waves)
    the planner can answer for 1 <= W <= 1024 at this height and batch size, and for oct, quad and quad_wide at least one
    hand-over to another form.  (Cases deselected from the test above are run here first.)"""
    for form in FORMS:
        for profile in PROFILES:
            if (form, profile) not in _RAN:
                _run_steps(torch_cuda, ctx, form, profile)
    for form in FORMS:
        assert _PLANNED[form] <= _LAUNCHED[form], (form, sorted(_PLANNED[form] - _LAUNCHED[form]))
        assert form in {lay for lay, _ in _LAUNCHED[form]}, (form, _LAUNCHED[form])
    for form in ("oct", "quad", "quad_wide"):
        assert {lay for lay, _ in _LAUNCHED[form]} - {form}, (form, _LAUNCHED[form])
    print("census: %s" % {f: sorted(v) for f, v in _LAUNCHED.items()})
    torch_cuda.cuda.empty_cache()


AUTO_ROWS = {1024: 2, 1016: 2, 1017: 2, 860: 2, 477: 3}     # 600 pictures: 1.7 .. 2.4 GB of records, planes and RGB


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("W", sorted(AUTO_ROWS))
def test_automatic_choice_on_long_rows(torch_cuda, ctx, W, profile):
    """layout = auto: one picture, nine, and 600 tiled on the device from five distinct ones"""
    H = AUTO_ROWS[W]
    params, rec, ref = _columns(W, H, profile, 5)
    for n in (1, 9, 600):
        got = _run(torch_cuda, ctx("auto"), params, rec, ref, n, ("auto", profile, W, H, n))
        print("automatic choice, %s, %d x %d, %d pictures: %s" % (profile, W, H, n, got))
    torch_cuda.cuda.empty_cache()


# ---- 2. columns and offsets in between ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _between(W):
    return _columns.__wrapped__(W, 6, "high", 5)


@functools.lru_cache(maxsize=None)
def _between_illegal(W):
    """modes whose neighbours are missing (predicted as 0) anywhere in the picture, QP 0 .. 51, chroma QP offsets at both ends"""
    return _with_oracle(*synth_packed(W, 6, 5, seed=W, profile="high", density="dense", qp_range=(0, 51), cqp_offsets=(-12, 12),
                                      illegal_modes=True, allow_qp36_i16=True))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("W", [255, 256, 257, 511, 513, 1023])
def test_columns_in_between(torch_cuda, ctx, form, W):
    hot = ctx(form)
    _run(torch_cuda, hot, *_between(W), 5, (form, W))
    if W == 257:
        _run(torch_cuda, hot, *_between_illegal(W), 5, (form, W, "illegal modes"))
    if W == 1023:     # planes-only reconstruction, then ycbcr_to_rgb_kernel on rows of 16 368 samples
        hot.set_fused_color(False)
        try:
            _run(torch_cuda, hot, *_between(W), 5, (form, W, "separate colour kernel"))
        finally:
            hot.set_fused_color(True)


# ---- 3. height ------------------------------------------------------------------------------------------------------------------
TALL = [(1, 1024), (2, 1024), (3, 1023), (5, 513)]


@functools.lru_cache(maxsize=None)
def _tall(W, H):
    return _with_oracle(*synth_packed(W, H, 5, seed=W * 2000 + H, profile="high", density="dense"))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("W,H", TALL)
def test_tall_pictures(torch_cuda, ctx, form, W, H):
    """passes (rows: 64 of 16 waves), bands (256 of four rows), tickets and seams (pipe with one-row bands: 1023 per picture)
    at their maxima: 1, 5 and 9 pictures, then 9 at every wave / row count the form is built for"""
    hot = ctx(form)
    params, rec, ref = _tall(W, H)
    for n in (1, 5, 9):
        assert _run(torch_cuda, hot, params, rec, ref, n, (form, W, H, n))[0] == form
    try:
        for waves in BUILT[form]:
            hot.set_waves_per_picture(waves)
            assert _run(torch_cuda, hot, params, rec, ref, 9, (form, W, H, "waves", waves)) == (form, waves)
    finally:
        hot.set_waves_per_picture(0)


def test_a_context_that_grows_and_shrinks(torch_cuda):
    """one context, the four banded forms in turn: 3 x 1024 (255 .. 1023 seams per picture), 1024 x 3 (seams of 1024 columns),
    20 x 17, 3 x 1024 again -- the seam buffer and the ticket bookkeeping grow and shrink between launches"""
    shapes = [_tall(3, 1024), _columns.__wrapped__(1024, 3, "high", 5), _tall(20, 17)]
    hot = HotPath(0)
    try:
        for form in ("wide", "quad_wide", "pipe", "pipe1"):
            hot.set_layout(form)
            for k in (0, 1, 2, 0):
                params, rec, ref = shapes[k]
                _run(torch_cuda, hot, params, rec, ref, 5, (form, int(params.width_mbs), int(params.height_mbs)))
    finally:
        hot.close()
    torch_cuda.cuda.empty_cache()


LARGE_H = 64


def test_one_large_picture(torch_cuda, ctx):
    """1024 x 64 macroblocks, High: the automatic choice, then one workgroup (rows) and sixteen bands (wide)"""
    t0 = time.perf_counter()
    params, rec, ref = _with_oracle(*synth_packed(1024, LARGE_H, 1, seed=64, profile="high", density="dense"))
    for form in ("auto", "rows", "wide"):
        got = _run(torch_cuda, ctx(form), params, rec, ref, 1, (form, 1024, LARGE_H))
        assert form == "auto" or got[0] == form, got
    print("one 1024 x %d picture, synthesis and oracle included: %.2f s" % (LARGE_H, time.perf_counter() - t0))
    torch_cuda.cuda.empty_cache()
