"""Layout of the guarded caller buffers of tests/test_gpu_recon_buffers.py -- plain arithmetic, TEST INFRASTRUCTURE, no device:
tests/test_recon_buffers_model.py checks it on the CPU, the GPU tests allocate by it.

One buffer is ONE allocation   front guard | payload | back guard   filled with SENTINEL, the payload included.  The payload
starts `off` bytes behind an address that is a multiple of PHASE (256: above every alignment a kernel could ask for and the
granule of the allocator), so that `off` is the payload's alignment phase whatever the allocator returned.  A guard is at least
eight pictures of the buffer: the short last group of the eight-picture form, were its stores not switched off, writes up to
seven whole pictures behind the payload -- inside the allocation, where it is seen; and at least 4096 bytes: a store at an
address rounded down to a 256-byte line, or a row flushed as whole 128-byte lines, stays inside it too."""
from minivideo_amd.hotpath import RECON_ALIGN

SENTINEL = 0xA5
PHASE = 256
OFFSETS = tuple(k * RECON_ALIGN for k in (0, 1, 3, 7, 15))   # the payload's phase: aligned to 256, and every odd multiple class
COUNTS = (1, 3, 5, 9)                                        # short groups of four and of eight; a full group of eight plus one
SHAPES = ((1, 1), (2, 1), (1, 2), (3, 2), (5, 3), (11, 9), (20, 17))   # macroblocks; widths 3 and 1 modulo the four-macroblock strip
BAND_SHAPES = tuple((w, h) for h in (4, 5, 9) for w in (2, 5))          # a band edge, one row past it, two bands plus a row
VARIED = ((5, 3), (11, 9))                                   # where the three buffers' phases vary independently


def guard_bytes(picture_bytes):
    return max(4096, 8 * int(picture_bytes))


def alloc_bytes(picture_bytes, n):
    """bytes of the allocation for n pictures: two guards, the payload, and room to move the payload to any phase"""
    return 2 * guard_bytes(picture_bytes) + int(n) * int(picture_bytes) + 2 * PHASE


def payload_start(base, picture_bytes, off):
    """offset of the payload inside an allocation that starts at address `base`"""
    assert 0 <= off < PHASE
    first = base + guard_bytes(picture_bytes)
    return (first + PHASE - 1) // PHASE * PHASE - base + off


def independent_offsets():
    """25 triples (packed, planes, RGB) of OFFSETS in which every pair of buffers takes every pair of phases"""
    k = len(OFFSETS)
    return [(OFFSETS[i], OFFSETS[j], OFFSETS[(i + j + 1) % k]) for i in range(k) for j in range(k)]
