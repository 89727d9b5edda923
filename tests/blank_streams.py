"""Test content for the picture scores (DESIGN.md 3 "Picture scores"): streams that mix "busy" and "blank" pictures, built from
one-picture generator streams -- each begins with its SPS and PPS, the corpus's "parameter sets before every picture" case.  The
generator's dense pictures score tens of thousands, its sparse ones hundreds to a few thousand; a picture's seed is advanced
until its score (oracle planes, tests/luma_ref.py) lies on its side of the gap, so that the tests' threshold (MIN_SCORE, i.e.
MINIVIDEO_BLANK_VARIANCE=1000) separates the two classes with room to spare.  The tests assert that again on what they use."""
import numpy as np

from minivideo_amd import gen
from minivideo_amd.hotpath import StreamParams
from oracle import loader
from tests import luma_ref as L

VARIANCE = 1000
MIN_SCORE = 16 * VARIANCE
BLANK_BELOW, BUSY_ABOVE = MIN_SCORE // 2, MIN_SCORE * 2


def mixed(wmb, hmb, busy, seed=5, profile="high", crop=None):
    """busy: one truth value per picture.  -> (stream, packed[n], planes[n] of the coded size, the whole-picture scores);
    crop: SPS frame-cropping offsets (left, right, top, bottom) for every picture"""
    parts, packed, planes, scores = [], [], [], []
    p = StreamParams(wmb, hmb, 0, 0, 0)
    for want in busy:
        for _ in range(64):
            seed += 1
            if crop is None:
                s, pk = gen.make_stream(wmb, hmb, 1, seed=seed, profile=profile, dense=bool(want))
            else:
                s, pk = gen.make_stream_crop(wmb, hmb, 1, [crop], seed=seed, profile=profile, dense=bool(want))
            yuv = loader.recon(p, pk[0], 1)[0].reshape(-1)
            sc = L.picture_score(yuv, wmb, hmb)
            if (sc > BUSY_ABOVE) if want else (sc < BLANK_BELOW):
                break
        else:
            raise AssertionError("the generator no longer makes %s pictures" % ("busy" if want else "blank"))
        parts.append(s)
        packed.append(pk[0])
        planes.append(yuv)
        scores.append(sc)
    return np.concatenate(parts), np.stack(packed), np.stack(planes), scores
