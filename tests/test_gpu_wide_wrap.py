"""GPU: the banded kernel forms (wide, quad_wide, pipe, pipe1) across the wraparound of the state that outlives a launch -- the
32-bit ticket counter, which is never reset (a workgroup's unit is atomicAdd(ticket, 1) - base, range-checked unsigned), and the
32-bit epoch tag of the seam granules (wide_prepare() in hotpath_abi.hip zeroes the seams and restarts at 1 when the tag comes
round, or granules left by epochs 1, 2, ... would count as fresh).  A busy context takes 2^32 tickets in about an hour and
2^32 launches in weeks; no test can wait for either, so two test hooks (mvhp_debug_set_wide_state / mvhp_debug_get_wide_state)
put a context where that many launches would have taken it and read the counter back:
* the counter passes 2^32 and 2^31 inside a launch: first, middle and last ticket of the launch, and the launch whose last
  ticket is 2^32 - 1; the launch after it;
* the epoch passes 2^32 with the seams full of another picture set's rows under the very tag that comes next; the same with
  a launch in flight on another stream, on the launch that grows the seam buffer, and together with the counter's wrap;
* after every launch here the counter on the device equals the host's mirror of it (one ticket per workgroup), and at the
  largest plans (1024 rows, 1023 seams per picture, short last groups) the mirror advanced by groups x bands.
Every launch is compared byte for byte, planes and RGB, with oracle/recon_ref.c; nothing here skews or corrupts the counter
(tests/test_gpu_wide.py::test_a_lost_unit_ends_the_launch_with_an_error does), and every wait in the kernels is bounded: a
defect ends a launch with the error word, which sync_check raises."""
import functools

import numpy as np
import pytest

from minivideo_amd import HotPath
from minivideo_amd.synth import synth_packed
from tests.test_gpu_extents import BUILT, _columns, _run, _tall
from tests.test_gpu_wide import WIDE, _oracle, _tile, torch_cuda  # noqa: F401  (torch_cuda: fixture)

pytestmark = pytest.mark.gpu

M32 = 1 << 32
EPOCH_LAST = 0xFFFFFFFF
PICTURES = {"wide": 1, "quad_wide": 4, "pipe": 4, "pipe1": 1}     # per group of workgroups (launch_plan.hip kernel_form())
D = 9                                                               # distinct pictures per set

# (form, W, H, rows per band, pictures): 20 x 17 in 5 bands of 4 rows (the last of one row) with 1, 5 and 9 pictures (short last
# groups on the four-picture forms); 3 x 41 for many seams per picture; the pipe forms in 17 bands of one row
CASES = ([(form, 20, 17, 4, n) for form in WIDE for n in (1, 5, 9)] + [(form, 3, 41, 4, 5) for form in WIDE]
         + [(form, 20, 17, 1, 9) for form in ("pipe", "pipe1")])
CASE_IDS = ["%s-%dx%d-rows%d-n%d" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def _set(W, H, which):
    """picture set "A" or "B" of W x H macroblocks: params, D records, the oracle's (planes, RGB) of each.  High, dense: about
    three macroblocks in four predict from the row above"""
    params, rec = synth_packed(W, H, D, seed=W * 100 + H + {"A": 0, "B": 5000}[which], profile="high", density="dense")
    return params, rec, _oracle(params, rec, D)


def _sets_differ_at_every_seam(W, H, rows, n):
    """what makes a stale seam visible: in every picture, at every band boundary, A and B differ in the sample line the seam
    carries (the last of the band above) and in the macroblock row that reads it (the first of the band below)"""
    (_, _, ref_a), (_, _, ref_b) = _set(W, H, "A"), _set(W, H, "B")
    for f in range(min(n, D)):
        ya = ref_a[f][0][:W * H * 256].reshape(H * 16, W * 16)
        yb = ref_b[f][0][:W * H * 256].reshape(H * 16, W * 16)
        for row in range(rows, H, rows):
            assert not np.array_equal(ya[row * 16 - 1], yb[row * 16 - 1]), (f, row)
            assert not np.array_equal(ya[row * 16:row * 16 + 16], yb[row * 16:row * 16 + 16]), (f, row)


class _Buffers:
    """records of n pictures tiled from a set, and zeroed outputs, on the device"""

    def __init__(self, torch, pictures, n):
        self.params, rec, self.ref = pictures
        self.n = n
        self.d_packed = _tile(torch, rec, n)
        self.d_yuv = torch.zeros(n * self.params.yuv_bytes, dtype=torch.uint8, device="cuda")
        self.d_rgb = torch.zeros(n * self.params.rgb_bytes, dtype=torch.uint8, device="cuda")

    def issue(self, hot, stream=None):
        hot.recon_dev(self.params, self.d_packed.data_ptr(), self.n, self.d_yuv.data_ptr(), self.d_rgb.data_ptr(), stream)

    def check(self, what):
        yuv, rgb = self.d_yuv.view(self.n, -1).cpu().numpy(), self.d_rgb.view(self.n, -1).cpu().numpy()
        for f in range(self.n):
            assert np.array_equal(yuv[f], self.ref[f % D][0]), (what, "planes", f)
            assert np.array_equal(rgb[f], self.ref[f % D][1]), (what, "RGB", f)


def _launch(torch, hot, pictures, n, want, what, stream=None):
    """one launch of n pictures into fresh buffers.  In this order: no error word; the form and band height asked for; the
    counter on the device equals the host's mirror (a launch whose bookkeeping is off stops the test HERE, before anything
    else is launched on its context); every byte.  -> the tickets the launch took, by the host's mirror"""
    buf = _Buffers(torch, pictures, n)
    torch.cuda.synchronize()
    base_before = hot.get_wide_state()[1]
    buf.issue(hot, stream)
    hot.sync_check(stream)
    assert hot.last_launch() == want, (what, hot.last_launch())
    dev, base, _, _ = hot.get_wide_state()
    assert dev == base, (what, "device counter %d, host mirror %d" % (dev, base))
    buf.check(what)
    return (base - base_before) % M32


def _context(form, rows):
    hot = HotPath(0)
    hot.set_layout(form)
    hot.set_waves_per_picture(rows)
    return hot


def _across(torch, case, bases_of):
    """the first launch of a fresh context, checked, tells the tickets T of the launch; then for each base of bases_of(T): set
    the counter, launch (B and A in turn), counter and mirror at base + T mod 2^32; launch again, at base + 2 T"""
    form, W, H, rows, n = case
    hot = _context(form, rows)
    try:
        T = _launch(torch, hot, _set(W, H, "A"), n, (form, rows), (case, "first"))
        assert T >= n and hot.get_wide_state()[:2] == (T, T), (case, T, hot.get_wide_state())
        print("tickets of a launch, %s: %d" % (case, T))
        for i, base in enumerate(bases_of(T)):
            epoch = hot.get_wide_state()[2]
            hot.set_wide_state(base, epoch)
            assert hot.get_wide_state()[:3] == (base, base, epoch)
            for k in (1, 2):
                pictures = _set(W, H, "AB"[(i + k) % 2])
                assert _launch(torch, hot, pictures, n, (form, rows), (case, base, k)) == T
                after = (base + k * T) % M32
                assert hot.get_wide_state()[:3] == (after, after, epoch + k), (case, base, k, hot.get_wide_state())
    finally:
        hot.close()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_ticket_counter_wraps_inside_a_launch(torch_cuda, case):
    """bases 2^32 - k: the first ticket of the launch is the last before the wrap (k = 1), the wrap in the middle, the last ticket
    alone behind it (k = T - 1), and the launch that ends on 2^32 - 1 and leaves the counter at exactly 0 (k = T)"""
    _across(torch_cuda, case, lambda T: [M32 - k for k in sorted({1, T // 2, T - 1, T})])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_ticket_counter_crosses_2_to_31(torch_cuda, case):
    """a signed compare, or a unit that does not survive its trip through an int in LDS, shows here"""
    _across(torch_cuda, case, lambda T: [(1 << 31) - T // 2])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_epoch_wrap_discards_stale_tags(torch_cuda, case):
    """set A at epoch 1 leaves its bottom rows in every seam under tag 1; the next launch, set B, comes after epoch 2^32 - 1 and
    runs at epoch 1 again: every byte must be B's.  Then epochs 2^32 - 2, 2^32 - 1, 1, 2 on one context, A and B in turn: B x n
    at epoch 1 of a fresh context, ONE picture at each of the two last epochs (the seams of pictures 1 .. n - 1 keep B's rows
    under tag 1), A x n at epoch 1, B x n at epoch 2"""
    form, W, H, rows, n = case
    _sets_differ_at_every_seam(W, H, rows, n)
    A, B = _set(W, H, "A"), _set(W, H, "B")
    hot = _context(form, rows)
    try:
        _launch(torch_cuda, hot, A, n, (form, rows), (case, "A at epoch 1"))
        dev, base, epoch, seam = hot.get_wide_state()
        assert epoch == 1
        hot.set_wide_state(base, EPOCH_LAST)
        _launch(torch_cuda, hot, B, n, (form, rows), (case, "B behind the wrap"))
        assert hot.get_wide_state()[2:] == (1, seam), hot.get_wide_state()
    finally:
        hot.close()
    hot = _context(form, rows)
    try:
        _launch(torch_cuda, hot, B, n, (form, rows), (case, "B at epoch 1"))
        hot.set_wide_state(hot.get_wide_state()[1], EPOCH_LAST - 2)
        for pictures, k, epoch in ((A, 1, EPOCH_LAST - 1), (B, 1, EPOCH_LAST), (A, n, 1), (B, n, 2)):
            _launch(torch_cuda, hot, pictures, k, (form, rows), (case, "epoch", epoch))
            assert hot.get_wide_state()[2] == epoch, (case, epoch, hot.get_wide_state())
    finally:
        hot.close()


@pytest.mark.parametrize("form", WIDE)
def test_epoch_wrap_behind_a_launch_in_flight_on_another_stream(torch_cuda, form):
    """70 pictures of A at epoch 2^32 - 1 on one stream and, with nothing waited for, 9 pictures of B on another: that launch
    zeroes the seams, which must not happen before the first one has finished with them"""
    torch = torch_cuda
    W, H, rows = 20, 17, 4
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    hot = _context(form, rows)
    try:
        _launch(torch, hot, _set(W, H, "A"), 70, (form, rows), (form, "A at epoch 1"))     # (the seam buffer has its size now)
        dev, base, _, seam = hot.get_wide_state()
        hot.set_wide_state(base, EPOCH_LAST - 1)
        first, second = _Buffers(torch, _set(W, H, "A"), 70), _Buffers(torch, _set(W, H, "B"), 9)
        torch.cuda.synchronize()     # (allocations and the tiling ran on torch's default stream)
        first.issue(hot, streams[0].cuda_stream)
        assert hot.last_launch() == (form, rows)
        second.issue(hot, streams[1].cuda_stream)
        assert hot.last_launch() == (form, rows)
        hot.sync_check(streams[0].cuda_stream)
        hot.sync_check(streams[1].cuda_stream)
        dev2, base2, epoch, seam2 = hot.get_wide_state()
        assert dev2 == base2 and (epoch, seam2) == (1, seam), (form, hot.get_wide_state())
        first.check((form, "A at epoch 2^32 - 1"))
        second.check((form, "B at epoch 1"))
    finally:
        hot.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("form", WIDE)
def test_epoch_wrap_on_the_launch_that_grows_the_seam_buffer(torch_cuda, form):
    hot = _context(form, 4)
    try:
        _launch(torch_cuda, hot, _set(20, 17, "A"), 1, (form, 4), (form, "one picture"))
        dev, base, epoch, seam = hot.get_wide_state()
        assert epoch == 1 and seam > 0
        hot.set_wide_state(base, EPOCH_LAST)
        _launch(torch_cuda, hot, _set(3, 41, "B"), 9, (form, 4), (form, "nine pictures of 3 x 41"))
        assert hot.get_wide_state()[2] == 1 and hot.get_wide_state()[3] > seam, (seam, hot.get_wide_state())
    finally:
        hot.close()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_both_wraps_in_one_launch(torch_cuda, case):
    form, W, H, rows, n = case
    _sets_differ_at_every_seam(W, H, rows, n)
    hot = _context(form, rows)
    try:
        T = _launch(torch_cuda, hot, _set(W, H, "A"), n, (form, rows), (case, "A at epoch 1"))
        hot.set_wide_state(M32 - T // 2, EPOCH_LAST)
        assert _launch(torch_cuda, hot, _set(W, H, "B"), n, (form, rows), (case, "B across both")) == T
        assert hot.get_wide_state()[:3] == (T - T // 2, T - T // 2, 1), (case, T, hot.get_wide_state())
        assert _launch(torch_cuda, hot, _set(W, H, "A"), n, (form, rows), (case, "A after both")) == T
    finally:
        hot.close()


# ---- the counter's invariant where the plans are largest (shapes and builders of tests/test_gpu_extents.py) ------------------------
@functools.lru_cache(maxsize=None)
def _long_rows():
    return _columns.__wrapped__(1024, 3, "high", 5)


def _counted(torch, hot, params, rec, ref, n, what):
    """one launch, every byte compared on the device (_run; plan == launch asserted there).  Then, in this order: counter on the
    device == host's mirror; the mirror advanced by groups x bands of the plan mvhp_plan_launch gave.  -> (form, rows)"""
    base_before = hot.get_wide_state()[1]
    form, rows = _run(torch, hot, params, rec, ref, n, what)
    dev, base, _, _ = hot.get_wide_state()
    assert dev == base, (what, "device counter %d, host mirror %d" % (dev, base))
    assert form in WIDE, (what, form)
    groups, bands = -(-n // PICTURES[form]), -(-int(params.height_mbs) // rows)
    assert (base - base_before) % M32 == groups * bands, (what, form, rows, base - base_before, groups, bands)
    return form, rows


@pytest.mark.parametrize("form", WIDE)
@pytest.mark.parametrize("W", [1, 3])
def test_counter_equals_its_mirror_on_tall_pictures(torch_cuda, form, W):
    """9 pictures of W x 1024 at every band height the form is built for: up to 1024 bands per picture, 3 groups of 4, 4 and 1"""
    params, rec, ref = _tall(W, 1024)
    hot = HotPath(0)
    try:
        hot.set_layout(form)
        for rows in BUILT[form]:
            hot.set_waves_per_picture(rows)
            assert _counted(torch_cuda, hot, params, rec, ref, 9, (form, W, 1024, rows)) == (form, rows)
    finally:
        hot.close()


@pytest.mark.parametrize("form", WIDE)
def test_counter_equals_its_mirror_on_long_rows(torch_cuda, form):
    """1 and 9 pictures of 1024 x 3, the band height left to the planner (quad_wide hands rows this long to wide)"""
    params, rec, ref = _long_rows()
    hot = HotPath(0)
    try:
        hot.set_layout(form)
        for n in (1, 9):
            _counted(torch_cuda, hot, params, rec, ref, n, (form, 1024, 3, n))
    finally:
        hot.close()
