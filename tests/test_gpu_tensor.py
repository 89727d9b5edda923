"""GPU: the tensor kernel (tensor_pack.hip, mvhp_tensor_dev) against the NumPy restatement (tests/tensor_ref.py), compared as raw
bytes -- the arithmetic is one fused multiply-add and one rounding, so there is no tolerance.  Every launch writes between two
64-byte sentinel bands.  Pictures from 2 x 2 to 258 wide and 258 tall (rows of 3 w bytes start on every byte phase), canvases equal
to the picture, one larger on each side (odd: 2-byte elements start on every even byte) and 224 x 224; all element types, layouts
and channel orders; constants that reach binary16 subnormals, binary16 infinity and negative values; a slot table with a
permutation, a skipped picture and a gap; every alignment the pointers may have; the widest and the tallest picture; a batch that
one launch does not hold; and the refused arguments."""
import numpy as np
import pytest

from minivideo_amd import HotPath
from minivideo_amd import hotpath as H
from minivideo_amd.hotpath import MiniVideoError
from tests import tensor_ref as R

pytestmark = pytest.mark.gpu

BAND = 64
FILL = 0xA5

SHAPES = ((2, 2, 1), (6, 4, 3), (34, 18, 3), (130, 66, 2), (258, 2, 1), (2, 258, 1))   # src_w, src_h, n
CONSTANTS = {
    "identity": ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
    "imagenet": R.constants(R.IMAGENET_MEAN, R.IMAGENET_STD),
    "subnormal": ((2.0 ** -20,) * 3, (0.0, 0.0, 0.0)),          # c * 2^-20 is a binary16 subnormal for every c below 64
    "overflow": ((1000.0, 1000.0, 1000.0), (0.0, 0.0, 0.0)),    # 66 and above pass 65504: binary16 infinity
    "negative": ((-0.0123, -1.5, -3e-5), (0.5, -0.25, 1e-3)),
}
PAD = (3, 200, 255)


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "no HIP device"
    return torch


@pytest.fixture(scope="module")
def hot():
    h = HotPath(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def tables():
    """the 256 x 3 values of every set of constants, made once"""
    return {k: R.value_table(*v) for k, v in CONSTANTS.items()}


@pytest.fixture(scope="module")
def pictures():
    """seeded random RGB of every shape, 0 and 255 among the samples; never written to"""
    out = {}
    for i, (w, h, n) in enumerate(SHAPES):
        a = np.random.default_rng(100 + i).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        a.reshape(-1)[:2] = (0, 255)
        a.setflags(write=False)
        out[(w, h)] = a
    return out


def _canvases(w, h):
    c = [None, (w + 1, h + 1)]
    if w <= 224 and h <= 224:
        c.append((224, 224))
    return c


def _run(torch, hot, rgb, params, slots=None, n_slots=None, out_phase=0, rgb_phase=0, n=None):
    """-> uint8 [n_slots, tensor bytes]: what the call left in a buffer filled with FILL; the bands around it are checked"""
    dev = torch.device("cuda", 0)
    n = rgb.shape[0] if n is None else n
    tb = H.tensor_bytes(params)
    ns = n if n_slots is None else n_slots
    src = torch.full((BAND + rgb_phase + rgb.size + BAND,), 0x5A, dtype=torch.uint8, device=dev)
    src[BAND + rgb_phase:BAND + rgb_phase + rgb.size] = torch.from_numpy(np.array(rgb).reshape(-1)).to(dev)
    out = torch.full((BAND + out_phase + ns * tb + BAND,), FILL, dtype=torch.uint8, device=dev)
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    d_slots = torch.tensor(slots, dtype=torch.int32, device=dev) if slots is not None else None
    torch.cuda.synchronize(dev)
    hot.tensor_dev(params, src.data_ptr() + BAND + rgb_phase, n, out.data_ptr() + BAND + out_phase,
                   d_slots.data_ptr() if d_slots is not None else None)
    hot.sync_check(None)
    raw = out.cpu().numpy()
    lo = BAND + out_phase
    assert (raw[:lo] == FILL).all() and (raw[lo + ns * tb:] == FILL).all(), "bytes around the tensors changed"
    return raw[lo:lo + ns * tb].reshape(ns, tb)


def _same(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
        assert False, (what, "first differing bytes", bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]], bad.size)


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("layout", [H.TENSOR_NCHW, H.TENSOR_NHWC])
@pytest.mark.parametrize("dtype", [H.TENSOR_F32, H.TENSOR_F16, H.TENSOR_BF16])
def test_every_shape_canvas_and_constant(hot, torch_cuda, tables, pictures, dtype, layout, bgr):
    for name, (scale, bias) in CONSTANTS.items():
        for (w, h), rgb in pictures.items():
            for canvas in _canvases(w, h):
                t = H.tensor_params(w, h, canvas, dtype, layout, bgr, PAD, scale, bias)
                got = _run(torch_cuda, hot, rgb, t)
                want = R.pack(rgb, canvas, dtype, layout, bgr, PAD, table=tables[name])
                _same(got, want, (name, w, h, canvas))


def test_subnormals_and_infinities_come_out(hot, torch_cuda, tables):
    """the values themselves, not only their agreement with the reference: binary16 subnormals stay subnormals (not flushed to
    zero), 1000 c overflows to infinity from c = 66 on, and a float32 subnormal survives the multiply-add"""
    rgb = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 16, 16, 3)
    sub = _run(torch_cuda, hot, rgb, H.tensor_params(16, 16, None, "float16", "nhwc", scale=(2.0 ** -20,) * 3)).view(np.float16)
    sub = sub.reshape(256, 3)[:, 0]
    assert (sub.view(np.uint16)[1:16] == np.arange(1, 16) * 16).all()        # c * 2^-20 = 16 c * 2^-24: subnormal bit patterns
    assert (sub[1:] != 0).all() and sub[0] == 0
    big = _run(torch_cuda, hot, rgb, H.tensor_params(16, 16, None, "float16", "nhwc", scale=(1000.0,) * 3)).view(np.float16)
    big = big.reshape(256, 3)[:, 1]
    assert np.isfinite(big[:66]).all() and np.isposinf(big[66:]).all() and big[65] == np.float16(64992)
    tiny = _run(torch_cuda, hot, rgb, H.tensor_params(16, 16, None, "float32", "nhwc", scale=(2.0 ** -149,) * 3)).view(np.uint32)
    assert (tiny.reshape(256, 3)[:, 2] == np.arange(256)).all()              # c * 2^-149: the float32 subnormal number c
    bf = _run(torch_cuda, hot, rgb, H.tensor_params(16, 16, None, "bfloat16", "nhwc", scale=(2.0 ** -133,) * 3)).view(np.uint16)
    assert (bf.reshape(256, 3)[:, 0] == np.arange(256)).all()                # c * 2^-133: the bfloat16 subnormal number c


@pytest.mark.parametrize("dtype,layout", [(H.TENSOR_F16, H.TENSOR_NCHW), (H.TENSOR_F32, H.TENSOR_NHWC), (H.TENSOR_BF16, H.TENSOR_NHWC)])
def test_slot_table(hot, torch_cuda, tables, pictures, dtype, layout):
    """a permutation, a skipped picture (-1) and a gap: slots nobody names keep the fill, also on an odd canvas, where a slot is
    210 or 420 bytes long and slots start on every even byte"""
    rgb = np.concatenate([pictures[(6, 4)], pictures[(6, 4)][:2][:, ::-1]])          # five pictures
    slots = [3, -1, 0, 6, 1]
    scale, bias = CONSTANTS["imagenet"]
    for canvas in (None, (7, 5)):
        t = H.tensor_params(6, 4, canvas, dtype, layout, False, PAD, scale, bias)
        got = _run(torch_cuda, hot, rgb, t, slots=slots, n_slots=8)
        want = R.pack(rgb, canvas, dtype, layout, False, PAD, table=tables["imagenet"])
        for i, s in enumerate(slots):
            if s >= 0:
                _same(got[s], want[i], (canvas, i, s))
        for s in (2, 4, 5, 7):
            assert (got[s] == FILL).all(), (canvas, s)


@pytest.mark.parametrize("dtype,layout", [(H.TENSOR_F16, H.TENSOR_NCHW), (H.TENSOR_F32, H.TENSOR_NCHW), (H.TENSOR_BF16, H.TENSOR_NHWC)])
def test_every_pointer_phase(hot, torch_cuda, tables, pictures, dtype, layout):
    """d_out on each 16-byte phase of a 64-byte line, d_rgb on each 4-byte phase of a 16-byte block: the bands stay untouched"""
    scale, bias = CONSTANTS["negative"]
    for (w, h), canvas in (((34, 18), (35, 19)), ((6, 4), None), ((2, 2), (3, 3))):
        rgb = pictures[(w, h)]
        t = H.tensor_params(w, h, canvas, dtype, layout, True, PAD, scale, bias)
        want = R.pack(rgb, canvas, dtype, layout, True, PAD, table=tables["negative"])
        for out_phase in (0, 16, 32, 48):
            for rgb_phase in (0, 4, 8, 12):
                _same(_run(torch_cuda, hot, rgb, t, out_phase=out_phase, rgb_phase=rgb_phase), want, (w, h, out_phase, rgb_phase))


@pytest.mark.parametrize("w,h", [(16384, 2), (2, 16384)])
def test_extents(hot, torch_cuda, tables, w, h):
    rgb = np.random.default_rng(w).integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    scale, bias = CONSTANTS["imagenet"]
    t = H.tensor_params(w, h, None, "float16", "nchw", False, PAD, scale, bias)
    _same(_run(torch_cuda, hot, rgb, t), R.pack(rgb, None, R.F16, R.NCHW, table=tables["imagenet"]), (w, h))


def test_more_pictures_than_one_launch_holds(hot, torch_cuda, tables):
    n = 65537
    rgb = np.random.default_rng(7).integers(0, 256, (n, 2, 2, 3), dtype=np.uint8)
    scale, bias = CONSTANTS["imagenet"]
    t = H.tensor_params(2, 2, None, "float16", "nchw", False, PAD, scale, bias)
    _same(_run(torch_cuda, hot, rgb, t), R.pack(rgb, None, R.F16, R.NCHW, table=tables["imagenet"]), n)


def test_any_strip_size_gives_the_same_bytes(hot, torch_cuda, tables, pictures):
    """forced rows per workgroup: one, odd ones, more than the canvas has, more than a workgroup's LDS holds of the source"""
    scale, bias = CONSTANTS["imagenet"]
    try:
        for (w, h), canvas, dtype, layout in (((34, 18), (35, 19), H.TENSOR_F16, H.TENSOR_NCHW), ((130, 66), (224, 224), H.TENSOR_BF16, H.TENSOR_NHWC),
                                              ((258, 2), None, H.TENSOR_F32, H.TENSOR_NCHW), ((2, 258), (3, 259), H.TENSOR_F16, H.TENSOR_NCHW)):
            rgb = pictures[(w, h)]
            t = H.tensor_params(w, h, canvas, dtype, layout, False, PAD, scale, bias)
            want = R.pack(rgb, canvas, dtype, layout, False, PAD, table=tables["imagenet"])
            for rows in (1, 2, 3, 7, 19, 64, 200, 1000, 16384):
                hot.set_tensor_rows(rows)
                _same(_run(torch_cuda, hot, rgb, t), want, (w, h, canvas, rows))
        with pytest.raises(MiniVideoError):
            hot.set_tensor_rows(-1)
        with pytest.raises(MiniVideoError):
            hot.set_tensor_rows(16385)
    finally:
        hot.set_tensor_rows(0)


def test_no_pictures_is_no_work(hot, torch_cuda, pictures):
    rgb = pictures[(6, 4)]
    got = _run(torch_cuda, hot, rgb, H.tensor_params(6, 4, (7, 5), "float16"), n=0, n_slots=3)
    assert (got == FILL).all()


def test_refusals(hot, torch_cuda, pictures):
    """every refused argument: MVHP_FAILURE with a message that names it, and not a byte written"""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    rgb = pictures[(6, 4)]
    src = torch.from_numpy(np.array(rgb).reshape(-1)).to(dev)
    src = torch.cat([src, torch.zeros(64, dtype=torch.uint8, device=dev)])
    out = torch.full((8192,), FILL, dtype=torch.uint8, device=dev)
    slots = torch.zeros(4, dtype=torch.int32, device=dev)
    good = dict(n=3, d_rgb=src.data_ptr(), d_out=out.data_ptr(), slots=None)

    def params(**kw):
        t = H.tensor_params(6, 4, (8, 8), "float16", "nchw")
        for k, v in kw.items():
            if k in ("scale", "bias"):
                getattr(t, k)[v[0]] = v[1]
            else:
                setattr(t, k, v)
        return t

    def refused(word, t=None, **kw):
        a = dict(good, **kw)
        with pytest.raises(MiniVideoError) as e:
            hot.tensor_dev(params() if t is None else t, a["d_rgb"], a["n"], a["d_out"], a["slots"])
        assert word in str(e.value), (word, str(e.value))

    hot.tensor_dev(params(), good["d_rgb"], 0, good["d_out"])   # (the good arguments are good)
    refused("dtype", params(dtype=3))
    refused("layout", params(layout=2))
    refused("flags", params(flags=2))
    refused("flags", params(flags=0x101))
    refused("src_w", params(src_w=0))
    refused("src_h", params(src_h=0))
    refused("src_w", params(src_w=16385, canvas_w=0, canvas_h=0))
    refused("src_h", params(src_h=16385, canvas_w=0, canvas_h=0))
    refused("canvas_w", params(canvas_w=16385))
    refused("canvas_h", params(canvas_h=16385))
    refused("canvas_w", params(canvas_w=5))
    refused("canvas_h", params(canvas_h=3))
    refused("canvas", params(canvas_w=0))
    refused("scale", params(scale=(1, float("inf"))))
    refused("bias", params(bias=(2, float("nan"))))
    refused("n =", n=-1)
    refused("d_rgb", d_rgb=None)
    refused("d_rgb", d_rgb=src.data_ptr() + 2)
    refused("d_out", d_out=None)
    refused("d_out", d_out=out.data_ptr() + 8)
    refused("d_slots", slots=slots.data_ptr() + 2)
    with pytest.raises(MiniVideoError) as e:
        hot.tensor_dev(None, good["d_rgb"], 3, good["d_out"])
    assert "parameters" in str(e.value)
    hot.sync_check(None)
    assert (out.cpu().numpy() == FILL).all()
