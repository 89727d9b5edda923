"""GPU: the directed corpus (tests/recon_directed.py) on every reconstruction form, planes and RGB byte for byte against
oracle/recon_ref.c (tests/test_recon_census.py asserts on the CPU that the oracle equals tests/spec_model.py on these batches, and
that the batches reach every cell of the content census for the pictures per wavefront and rows per band used here).

Every batch of every setting runs on the forced form -- the launch is asserted to be that form --
* at each wave count the form is built for (banded forms: each rows per band, which the launch must then report),
* with fused RGB, with the separate colour stage and with planes only (an RGB buffer that is not passed stays untouched),
* and, fused, rotated by one picture as many times as a wavefront holds pictures, so that every picture visits every index of its
  group whatever the census makes of the records."""
import numpy as np
import pytest

from minivideo_amd.hotpath import STAGE_COLOR, STAGE_RECON
from tests import recon_directed as D
from tests.test_gpu_extents import BUILT
from tests.test_recon_census import expected

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
# (setting, family) pairs that have batches: the zero family is the parity setting's, spec_pcm is the spec corpus -- which runs under
# "spec" -- plus its own I_PCM batches
CASES = (("parity", "positional"), ("parity", "zero"), ("parity", "wave"), ("spec", "positional"), ("spec", "wave"),
         ("spec_pcm", "wave_pcm"))


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "no HIP device"
    return torch


@pytest.fixture
def form(request, hot):
    """the layout the `hot` context of this test was made with"""
    return request.node.callspec.params["hot"]


_ON_DEVICE = {}


def _device_batch(torch, setting, index):
    key = (setting, index)
    if key not in _ON_DEVICE:
        b = D.corpus(setting)[index]
        yuv, rgb = expected(setting, index)
        _ON_DEVICE[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (b.rec.reshape(b.rec.shape[0], -1), yuv, rgb))
    return _ON_DEVICE[key]


def _differ(got, want, what):
    bad = np.nonzero(got.cpu().numpy().reshape(-1) != want.cpu().numpy().reshape(-1))[0]
    per = want.shape[1]
    raise AssertionError("%s: %d bytes differ from the oracle; first in picture %d at offset %d" % (what, bad.size, bad[0] // per, bad[0] % per))


def _run(torch, hot, form, params, rec, yuv, rgb, how, waves, what):
    """one launch; how: "fused" (mvhp_recon_batch_dev with an RGB buffer), "separate" (reconstruction, then the colour stage) or
    "planes" (no RGB buffer)"""
    n = rec.shape[0]
    d_yuv = torch.full_like(yuv, SENTINEL)
    d_rgb = torch.full_like(rgb, SENTINEL)
    torch.cuda.synchronize()
    plan = hot.plan_launch(params, n)
    if how == "separate":
        hot.set_fused_color(False)
        try:
            hot.recon_stages_dev(params, rec.data_ptr(), n, d_yuv.data_ptr(), d_rgb.data_ptr(), None, STAGE_RECON | STAGE_COLOR)
        finally:
            hot.set_fused_color(True)
    else:
        hot.recon_dev(params, rec.data_ptr(), n, d_yuv.data_ptr(), d_rgb.data_ptr() if how == "fused" else None, None)
    hot.sync_check(None)
    what = "%s, %s, %s colour, waves %s" % (form, what, how, waves)
    assert hot.last_launch() == plan and plan[0] == form, (what, hot.last_launch(), plan)
    assert waves is None or plan[1] == waves, (what, plan)
    if not torch.equal(d_yuv, yuv):
        _differ(d_yuv, yuv, what + ", planes")
    if how == "planes":
        assert bool((d_rgb == SENTINEL).all()), what + ": an RGB buffer that was not passed was written"
    elif not torch.equal(d_rgb, rgb):
        _differ(d_rgb, rgb, what + ", RGB")


@pytest.mark.parametrize("setting,family", CASES)
def test_directed_corpus(hot, form, torch_cuda, setting, family):
    torch = torch_cuda
    group = max(D.FORMS[form][0], 1)
    ran = 0
    try:
        for index, b in enumerate(D.corpus(setting)):
            if b.family != family:
                continue
            rec, yuv, rgb = _device_batch(torch, setting, index)
            for waves in BUILT[form]:
                hot.set_waves_per_picture(waves)
                for how in ("fused", "separate", "planes"):
                    # a banded form runs exactly the rows per band asked for; the others step down to what the picture has rows for
                    _run(torch, hot, form, b.params, rec, yuv, rgb, how, waves if form in D.BANDED else None, b.name)
            hot.set_waves_per_picture(0)
            for turn in range(1, group + 1):
                r, y, c = (torch.roll(t, turn, 0).contiguous() for t in (rec, yuv, rgb))
                _run(torch, hot, form, b.params, r, y, c, "fused", None, "%s rotated by %d" % (b.name, turn))
            ran += 1
    finally:
        hot.set_waves_per_picture(0)
    assert ran == sum(1 for b in D.corpus(setting) if b.family == family) and ran > 0


def test_cases_leave_no_batch_out():
    for setting in D.SETTINGS:
        for b in D.corpus(setting):
            assert (setting, b.family) in CASES or (setting == "spec_pcm" and ("spec", b.family) in CASES), (setting, b.name)
