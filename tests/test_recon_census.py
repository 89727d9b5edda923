"""CPU: the content census (tests/recon_census.py) and the directed corpus (tests/recon_directed.py).

* the rule-built universe has the sizes counted by hand on 1 x 1 and 2 x 1;
* the directed corpus reaches EVERY cell of the universe, for every (setting, pictures per wavefront, rows per band) that
  tests/test_gpu_recon_census.py runs -- each shape for the cells that carry a position, the corpus as a whole for those that do not;
* no batch is slack: without any one of them some cell is missed (a census that found everything everywhere would pass the
  coverage test with any corpus; it cannot pass this one);
* the expectation of the GPU file does not rest on the oracle alone: oracle/recon_ref.c = tests/spec_model.py on the whole corpus
  (luma_dc_from = 37 for the parity setting).  The "zero" family cannot be modelled -- the standard forbids those pictures and the
  model refuses them, which is asserted; the reference's "predict 0" there is pinned by the oracle's own tests."""
import functools
from collections import Counter

import numpy as np
import pytest

from oracle import loader
from tests import recon_census as RC
from tests import recon_directed as D
from tests import spec_model as M

COMBOS = sorted({(g, r) for g, rows in D.FORMS.values() for r in rows})


def test_forms_table_matches_the_built_sizes():
    from tests.test_gpu_extents import BUILT
    assert set(D.FORMS) == set(BUILT)
    for form in D.BANDED:
        assert D.FORMS[form][1] == BUILT[form], form          # banded forms: BUILT holds the rows per band
    assert (8, 0) in COMBOS and (4, 8) in COMBOS and (1, 1) in COMBOS and len(COMBOS) == 10


def test_universe_sizes_counted_by_hand():
    """1 x 1: column "only", row "first", no neighbour at all.
    Intra4x4: block 0 has nothing -> DC only; blocks 1, 4, 5 (top row) have left -> DC, H, HU; blocks 2, 8, 10 (left column) have
    above (+ above right substituted) -> DC, V, DDL, VL; the other nine have everything -> 9 modes: (1 + 3 * 3 + 3 * 4 + 9 * 9) * 2
    coded = 206.  Intra8x8: (1 + 3 + 4 + 9) * 2 = 34.  Intra16x16: DC x 3 luma x 2 = 6.  Chroma: DC x 3 = 3."""
    ex = {}
    u = RC.positional_universe("spec", 1, 1, 4, ex)
    by = Counter(t[0] for t in u)
    assert by == {"i4": 206, "i8": 34, "i16": 6, "chroma": 3} and len(u) == 249
    # what the rules removed from the 18 classes x 396 cells: 17 classes the shape does not have, and the modes above
    assert sum(ex.values()) + len(u) == 18 * 396
    print("1x1 spec exclusions:", ex)
    # parity adds the "predict 0" cells: Intra4x4 block patterns (left, above, corner missing) (1,1,1): 8 modes; (0,1,1): 6;
    # (1,0,1): 5; Intra8x8 the same three patterns: 19 + 19; Intra16x16 V, H, Plane and chroma H, V, Plane with (1, 1): 3 + 3
    z = RC.positional_universe("parity", 1, 1, 4) - u
    assert Counter(t[1] for t in z) == {"i4": 19, "i8": 19, "i16": 3, "chroma": 3}
    # 2 x 1: columns "first" and "last", row "first".  "last" has its left neighbour: Intra4x4 blocks 0, 1, 4, 5 -> 3 modes, the
    # rest 9: (4 * 3 + 12 * 9) * 2 = 240; Intra8x8 (2 * 3 + 2 * 9) * 2 = 48; Intra16x16 DC, H: 12; chroma DC, H: 6
    u2 = RC.positional_universe("spec", 2, 1, 4)
    assert Counter(t[0] for t in u2 if t[1] == "last") == {"i4": 240, "i8": 48, "i16": 12, "chroma": 6}
    assert len(u2) == 249 + 306
    # the cells without a position: 3 x 52 QP'Y, 2 x 40 QPc, 4 clips; groups of eight, parity: 10 conditions x (none + all + 8, + 7, + 1
    # = 10 + 9 + 3) + (4 + 8) combinations x 3 lengths
    f = RC.free_universe("parity", 8)
    assert len(f) == 156 + 80 + 4 + 10 * 22 + 36
    assert len(RC.free_universe("spec", 4)) == 156 + 80 + 4 + 9 * (6 + 5 + 3) + 36
    assert len(RC.free_universe("spec", 1)) == 156 + 80 + 4 + 14


@functools.lru_cache(maxsize=None)
def _parts(setting):
    """per batch: (W, H), raw positional cells, cells without a position, wave cells per group size"""
    out = []
    for b in D.corpus(setting):
        pos, free = RC.raw_cells(b.params, b.rec)
        waves = {g: RC.wave_cells(b.params, b.rec, g) for g in (1, 4, 8)}
        out.append(((int(b.params.width_mbs), int(b.params.height_mbs)), pos, free, waves))
    return out


def _missing(setting, group, rpb, leave_out=None):
    """the cells of the universe the corpus (without batch `leave_out`) does not reach"""
    parts = [p for i, p in enumerate(_parts(setting)) if i != leave_out]
    free = set().union(*[p[2] | p[3][group] for p in parts])
    miss = sorted(RC.free_universe(setting, group) - free, key=repr)
    for (W, H) in D.shapes_of(setting):
        got = set().union(*[RC.classed(p[1], W, rpb) for p in parts if p[0] == (W, H)])
        miss += [((W, H),) + t for t in sorted(RC.positional_universe(setting, W, H, rpb) - got, key=repr)]
    return miss


@pytest.mark.parametrize("setting", D.SETTINGS)
def test_census_is_the_sum_of_its_parts(setting):
    """census() -- the entry point -- gives what the cached parts give, on a batch of each family"""
    seen = set()
    for b, (shape, pos, free, waves) in zip(D.corpus(setting), _parts(setting)):
        if (b.family, shape) in seen:
            continue
        seen.add((b.family, shape))
        for g, r in ((8, 0), (4, 4), (1, 2)):
            assert RC.census(b.params, b.rec, g, r) == RC.classed(pos, shape[0], r) | free | waves[g], b.name


@pytest.mark.parametrize("setting", D.SETTINGS)
def test_directed_corpus_covers_the_universe(setting):
    for group, rpb in COMBOS:
        miss = _missing(setting, group, rpb)
        assert not miss, "%s, %d pictures per wavefront, %d rows per band: %d cells missed, first %r" % (
            setting, group, rpb, len(miss), miss[:8])
    assert all(b.rec.shape[0] <= 17 for b in D.corpus(setting))


@pytest.mark.parametrize("setting", D.SETTINGS)
def test_no_batch_is_slack(setting):
    for i, b in enumerate(D.corpus(setting)):
        if setting == "spec_pcm" and b.family != "wave_pcm":
            continue                                           # (the spec setting's own batches: answered for under "spec")
        assert any(_missing(setting, g, r, leave_out=i) for g, r in ((8, 0), (4, 4), (1, 4))), \
            "the census does not notice that %r is gone" % b.name


@functools.lru_cache(maxsize=None)
def expected(setting, index):
    """(planes[n, -1], RGB[n, -1]) of batch `index`: oracle/recon_ref.c"""
    b = D.corpus(setting)[index]
    n = b.rec.shape[0]
    yuv, rgb = loader.recon(b.params, b.rec, n, want_rgb=True)
    return yuv.reshape(n, -1), rgb.reshape(n, -1)


@pytest.mark.parametrize("setting", D.SETTINGS)
def test_oracle_equals_model_on_the_whole_corpus(setting):
    done = refused = 0
    for i, b in enumerate(D.corpus(setting)):
        if setting == "spec_pcm" and b.family != "wave_pcm":
            continue                                       # (the spec setting's own batches: modelled under "spec")
        yuv = expected(setting, i)[0]
        for k in range(b.rec.shape[0]):
            if b.family == "zero":                      # (a picture of the walk that happens to be legal is modelled like the rest)
                try:
                    M.reconstruct(b.params, b.rec[k], 37)
                except M.SpecModelError:
                    refused += 1
                    continue
            got = M.reconstruct(b.params, b.rec[k], 36 if setting != "parity" else 37)
            assert M.dc_from(b.params) == (36 if setting != "parity" else 37)
            assert got.cls.max() == M.CONFORMANT or got.defect.any(), (b.name, k)
            assert np.array_equal(got.yuv, yuv[k]), "%s picture %d: oracle and model differ" % (b.name, k)
            done += 1
    assert done and (refused > 100) == (setting == "parity")
