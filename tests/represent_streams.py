"""Test content for the representative pictures (DESIGN.md 3 "Representative pictures"): streams put together from one-picture
generator streams -- each begins with its SPS and PPS -- in which a slot's candidates are a few distinct pictures, some of them
repeated.  A picture that occurs several times among the candidates pulls the mean histogram onto itself, so the reference rule
(tests/hist_ref.py over the oracle's planes) picks its first occurrence -- its copies tie exactly, the earliest wins -- and every
other picture is at least twice as far from the mean; scenario() asserts that margin, and
that the "busy" and "blank" pictures lie on their sides of the blank threshold (tests/blank_streams.py), before anything else
looks at the stream."""
import numpy as np

from minivideo_amd import gen
from minivideo_amd.hotpath import StreamParams
from oracle import loader
from tests import blank_streams as B, hist_ref as R, luma_ref as L

W, H = 8, 6
RECT = (0, 0, 16 * W, 16 * H)
MARGIN = 2          # every other picture among the candidates is at least this many times as far from the mean as the winner

# name: (the pictures of the stream by letter -- capitals are busy (dense) pictures, small letters blank (sparse) ones --,
#        -n, the IDR every slot's file must hold under MINIVIDEO_REPRESENTATIVE=1, and under -b as well)
SCENARIOS = {
    "outlier": ("pBAAAAA", 1, [2], [2]),          # the primary looks like nothing else: the first of the five alike wins
    "second_slot": ("CpBAAAAA", 2, [0, 3], [0, 3]),   # slot 0 has no alternates (slot 1 follows at once); slot 1 as above
    "primary_wins": ("ABAA", 1, [0], [0]),        # the primary is the repeated picture: pass 3 has nothing to do
    "blank_majority": ("AbbbC", 1, [1], [0]),     # three blank pictures win the vote; under -b they are not eligible, A and C
                                                  # are two candidates, and the first -- the primary -- stays
    "all_slots": ("ABC", 3, [0, 1, 2], [0, 1, 2]),   # every picture is a slot: no alternates, no pass 2
}
_CACHE = {}


def _picture(letter, seed):
    """-> (one-picture stream, its oracle planes, its score, the seed behind it): busy for a capital, blank for a small letter"""
    busy = letter.isupper()
    p = StreamParams(W, H, 0, 0, 0)
    for _ in range(64):
        seed += 1
        s, pk = gen.make_stream(W, H, 1, seed=seed, profile="high", dense=busy)
        yuv = loader.recon(p, pk[0], 1)[0].reshape(-1)
        sc = L.picture_score(yuv, W, H)
        if (sc > B.BUSY_ABOVE) if busy else (sc < B.BLANK_BELOW):
            return s, yuv, sc, seed
    raise AssertionError("the generator no longer makes %s pictures" % ("busy" if busy else "blank"))


def scenario(name):
    """-> (stream, planes[n], scores[n], records[n]) of SCENARIOS[name], checked against the reference rule"""
    if name in _CACHE:
        return _CACHE[name]
    letters, n, final, final_b = SCENARIOS[name]
    made, seed = {}, 40
    for c in letters:
        if c not in made:
            made[c] = _picture(c, seed)
            seed = made[c][3]
    stream = np.concatenate([made[c][0] for c in letters])
    planes = np.stack([made[c][1] for c in letters])
    scores = [made[c][2] for c in letters]
    recs = R.records(planes, len(letters), W, H, RECT)
    assert len({made[c][1].tobytes() for c in made}) == len(made)                 # distinct letters are distinct pictures
    # the reference rule alone, slot by slot (unfiltered: slot k is IDR k, only the last slot has alternates, at most 8)
    for k in range(n):
        cand = [k] + (list(range(n, len(letters)))[:8] if k == n - 1 else [])
        for eligible, want in ((None, final[k]), ([scores[i] >= B.MIN_SCORE for i in cand], final_b[k])):
            got = cand[R.choose(recs[cand], eligible)]
            assert got == want, (name, k, got, want)
            live = [i for j, i in enumerate(cand) if eligible is None or eligible[j]]
            if len(live) > 2:
                d = dict(zip(live, R.distances([R.bins(recs[i]) for i in live])))
                others = [v for i, v in d.items() if planes[i].tobytes() != planes[want].tobytes()]
                assert not others or min(others) >= MARGIN * max(d[want], 1), (name, k, d)
    _CACHE[name] = (stream, planes, scores, recs)
    return _CACHE[name]
