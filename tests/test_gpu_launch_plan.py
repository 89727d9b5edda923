"""GPU: the launch planner against what is launched.  mvhp_plan_launch(ctx, NULL, ...) asked BEFORE a reconstruction launch must
name the form and the wave count mvhp_last_launch_info reports AFTER it -- on whatever device this runs on (tests/
test_launch_plan.py pins the policy itself for described devices, without a GPU) -- and the launch's planes are the oracle's."""
import numpy as np
import pytest

from minivideo_amd import HotPath
from minivideo_amd.hotpath import LAYOUTS, PARAM_MAY_HAVE_8X8
from minivideo_amd.synth import synth_packed
from oracle import loader

pytestmark = pytest.mark.gpu

DISTINCT = 5


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def pictures():
    """per shape: params, records and the oracle's planes of DISTINCT High pictures (tiled up to the batch size)"""
    out = {}
    for (W, H) in [(5, 4), (20, 17)]:
        params, rec = synth_packed(W, H, DISTINCT, seed=W * 10 + H, profile="high", density="dense")
        out[(W, H)] = (params, rec, [loader.recon(params, rec[k], 1)[0].reshape(-1) for k in range(DISTINCT)])
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
def test_plan_equals_launch(torch_cuda, pictures, layout):
    torch = torch_cuda
    hot = HotPath(0)
    try:
        hot.set_layout(layout)
        for (W, H), (params, rec, ref) in pictures.items():
            d_small = torch.from_numpy(rec.reshape(DISTINCT, -1)).cuda()
            for n in (1, 5, 300):
                d_packed = d_small.repeat((n + DISTINCT - 1) // DISTINCT, 1)[:n].contiguous()
                d_yuv = torch.zeros(n * params.yuv_bytes, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                for flags in (0, PARAM_MAY_HAVE_8X8):   # (a hint for the planner only: every kernel reconstructs Intra8x8)
                    params.flags = flags
                    d_yuv.zero_()
                    torch.cuda.synchronize()
                    plan = hot.plan_launch(params, n)
                    hot.recon_dev(params, d_packed.data_ptr(), n, d_yuv.data_ptr(), None, None)
                    hot.sync_check(None)
                    assert hot.last_launch() == plan, (layout, W, H, n, flags)
                    assert layout == "auto" or plan[0] == layout, plan   # (no slices, line buffers fit: a forced form runs)
                    yuv = d_yuv.view(n, -1).cpu().numpy()
                    for f in range(n):
                        assert np.array_equal(yuv[f], ref[f % DISTINCT]), (layout, W, H, n, flags, f)
                del d_packed, d_yuv
    finally:
        hot.close()
    torch.cuda.empty_cache()
