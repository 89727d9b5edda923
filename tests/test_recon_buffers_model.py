"""CPU: the arithmetic tests/test_gpu_recon_buffers.py rests on (tests/recon_buffers.py), and the facts the alignment rule of the
reconstruction entry points (MVHP_RECON_ALIGN, include/minivideo_hotpath.h) needs from the callers inside the library: the
per-picture sizes are multiples of it, so picture k of an aligned buffer is aligned.  No device, nothing launched."""
import itertools

import pytest

from minivideo_amd import hotpath
from minivideo_amd.hotpath import LAYOUTS, RECON_ALIGN, PlanDevice, StreamParams, plan_launch
from tests import recon_buffers as B

PER_MB = {"packed_bytes": 800, "yuv_bytes": 384, "rgb_bytes": 768}
ALL_SHAPES = tuple(dict.fromkeys(B.SHAPES + B.BAND_SHAPES + ((7, 5), (2, 17), (2, 5))))


def test_python_and_library_agree_on_the_alignment():
    assert hotpath.lib().mvhp_recon_align() == RECON_ALIGN == 16
    assert RECON_ALIGN & (RECON_ALIGN - 1) == 0 and B.PHASE % RECON_ALIGN == 0
    assert B.OFFSETS == (0, 16, 48, 112, 240) and max(B.OFFSETS) < B.PHASE


@pytest.mark.parametrize("W,H", ALL_SHAPES)
def test_payload_phase_and_guards(W, H):
    p = StreamParams(W, H, 0, 0, 0)
    for name, per_mb in PER_MB.items():
        pic = getattr(p, name)
        assert pic == W * H * per_mb
        guard = B.guard_bytes(pic)
        assert guard >= 8 * pic and guard >= 4096
        for n, off in itertools.product(B.COUNTS + (513,), B.OFFSETS):
            total = B.alloc_bytes(pic, n)
            # the allocator's own alignment must not matter: every base address modulo the phase, and a few odd ones
            for base in list(range(0, 2 * B.PHASE, 16)) + [1, 7, 4097, (1 << 40) + 24]:
                start = B.payload_start(base, pic, off)
                assert (base + start) % B.PHASE == off
                assert start >= guard                                  # front guard
                assert total - (start + n * pic) >= guard              # back guard
                # every picture of the payload is on the rule's alignment
                assert all((base + start + k * pic) % RECON_ALIGN == 0 for k in (0, 1, n - 1))


def test_independent_offsets_cover_every_pair():
    trip = B.independent_offsets()
    assert len(trip) == 25
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert {(t[a], t[b]) for t in trip} == set(itertools.product(B.OFFSETS, B.OFFSETS))


def test_picture_sizes_are_multiples_of_the_alignment():
    """what the library's own callers rely on (picture k of a batch buffer = base + k x picture size): 800, 384 and 768 bytes
    per macroblock, at the corners of 1 .. 1024 macroblocks each way and at the shapes the GPU tests use"""
    L = hotpath.lib()
    shapes = list(itertools.product((1, 2, 3, 1023, 1024), repeat=2)) + list(ALL_SHAPES)
    for W, H in shapes:
        p = StreamParams(W, H, 0, 0, 0)
        for name, f in (("packed_bytes", L.mvhp_packed_frame_bytes), ("yuv_bytes", L.mvhp_yuv_frame_bytes),
                        ("rgb_bytes", L.mvhp_rgb_frame_bytes)):
            assert getattr(p, name) == f(p) == W * H * PER_MB[name]
            assert getattr(p, name) % RECON_ALIGN == 0
        # the engine's compact slot (decode_engine.cpp compact_slot_bytes): the format's bound rounded up to 16
        slot = (W * H * 804 + 1536 + 15) & ~15
        assert slot % RECON_ALIGN == 0 and slot % 4 == 0
    assert all(v % RECON_ALIGN == 0 for v in PER_MB.values())


@pytest.mark.parametrize("form", LAYOUTS[1:])
def test_no_form_hands_these_shapes_over(form):
    """on a device of 256 CUs and 160 KiB of LDS a forced form keeps every shape of the GPU tests (the planner hands over only
    what does not fit a form's line buffers or 32-bit offsets, or carries slices / scaling matrices): the GPU tests may assert
    the forced form as the launched one"""
    for (W, H), n, flags in itertools.product(ALL_SHAPES, B.COUNTS + (513,), (0, hotpath.PARAM_MAY_HAVE_8X8, hotpath.PARAM_DEBLOCK)):
        got = plan_launch(PlanDevice(256, 160 * 1024, LAYOUTS.index(form), 0), StreamParams(W, H, 0, 0, flags), n)
        assert got is not None and got[0] == form, (W, H, n, flags, got)
