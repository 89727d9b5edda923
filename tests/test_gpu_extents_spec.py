"""GPU: spec mode at the widest and tallest pictures (tests/test_gpu_extents.py does the same outside spec mode).  Pictures of
several slices and scaling matrices run on the EXT instantiations of "rows", "wide" and "pipe1", code paths of their own: 1024
columns in one and two rows, 1024 rows of one and three macroblocks, slice boundaries in mid band, one slice per row and one per
macroblock, random weights, I_PCM, chroma QP offsets -- planes against the model of the standard (tests/spec_model.py), RGB
against the oracle's, the launch form asserted.  I_PCM in column 1023 and in row 1023 runs through all seven forms.
The modelled pictures are computed once per session."""
import functools

import numpy as np
import pytest

from tests import spec_model as M
from tests import spec_synth as S
from tests.test_gpu_spec_model import FORMS, _check, _modelled

pytestmark = pytest.mark.gpu

SHAPES = [(1024, 1), (1024, 2), (1, 1024), (3, 1024)]


@pytest.fixture(scope="module", params=FORMS)
def spec_hot(request):
    from minivideo_amd import HotPath
    h = HotPath(0)
    h.set_layout(request.param)
    h.form = request.param
    yield h
    h.close()


@functools.lru_cache(maxsize=None)
def _extent(W, H):
    p, rec, ids, cls = S.spec_pictures(W, H, ["band_mid", "per_row", "per_mb"], seed=W + H, weight_set="random", pcm_share=0.1,
                                       cqp=(5, -7))
    assert not (cls == M.BEYOND).any()
    assert p.flags & M.SLICES and p.flags & M.SCALING and len(np.unique(ids[2])) == W * H
    return p, rec, _modelled(p, rec)


@pytest.mark.parametrize("W,H", SHAPES)
def test_slices_and_scaling_at_the_extents(spec_hot, W, H):
    p, rec, want = _extent(W, H)
    _check(spec_hot, spec_hot.form, p, rec, want, "%dx%d" % (W, H))


@functools.lru_cache(maxsize=None)
def _pcm_at_the_edge(W, H):
    """five pictures (a short group for the four- and eight-picture forms) with I_PCM macroblocks in the last column (W = 1024) or
    the last row (H = 1024) beside the random ones: alone, above / beside each other, and beside a predicted macroblock"""
    F = 5
    p, rec, ids, cls = S.spec_pictures(W, H, ["one"] * F, seed=90 + W, pcm_share=0.02, qp_range=(34, 38), cqp=(2, -3),
                                       spec_luma_dc=True, force_scaling=False)
    assert not p.flags & (M.SLICES | M.SCALING) and p.flags & 2
    rng = np.random.default_rng(W)
    for k in range(F):
        where = np.zeros(W * H, bool)
        if W == 1024:
            where[(k % H) * W + 1023] = True           # column 1023, first / second row in turn
            if k >= 3:
                where[W * H - 1] = where[1023] = True  # ... both rows
            if k == 2:
                where[W * H - 2] = True                # ... and its left neighbour
        else:
            where[1023 * W + k % W] = True             # row 1023
            if k >= 3:
                where[1023 * W:] = True                # ... the whole row
            if k == 2:
                where[1022 * W + k % W] = True         # ... and the macroblock above
        S.set_pcm(rec[k], where, rng)
        S.fix_nz_mask(rec[k])
    assert (rec[:, -1 if H == 1024 else 1023, 0] == M.IPCM).sum() >= 3
    return p, rec, _modelled(p, rec)


@pytest.mark.parametrize("W,H", [(1024, 2), (2, 1024)])
def test_pcm_in_the_last_column_and_row_on_every_form(hot, W, H):
    """(a forced four- or eight-picture form hands a 1024-column picture to a simpler one: the form asserted is the planned one)"""
    p, rec, want = _pcm_at_the_edge(W, H)
    plan = hot.plan_launch(p, rec.shape[0])
    _check(hot, plan[0], p, rec, want, "I_PCM at the edge of %dx%d" % (W, H))
    assert hot.last_launch() == plan
