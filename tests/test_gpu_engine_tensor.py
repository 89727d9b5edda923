"""GPU: the decode engine with MVHP_OUT_TENSOR (Engine.set_tensor, Engine.decode(..., tensor=True), Engine.decode_tensors) on
generator streams.  Host delivery: every delivered tensor equals the restatement (tests/tensor_ref.py) of the RGB the same request
delivers with MVHP_OUT_RGB_ONLY, byte for byte, and d2h_bytes is exactly the tensors' bytes.  Device delivery: decode_tensors on an
engine of one context equals the host-delivered tensors; failed and over-range pictures leave zeros and ok = False; a picture past
the target's last slot fails and touches nothing.  Refused: device delivery on two contexts, tensors together with JPEG, PNG or
the black-bar probe, and a tensor call without a request."""
import ctypes as C

import pytest

from minivideo_amd import Engine, gen
from minivideo_amd import hotpath as H
from tests import tensor_ref as R
from tests.test_engine_harness import _break_picture
from tests.util import Stream

pytestmark = pytest.mark.gpu

WMB, HMB, F = 6, 5, 7
CROP = (1, 3, 2, 1)
BROKEN = 3
SCALE, BIAS = R.constants(R.IMAGENET_MEAN, R.IMAGENET_STD)
PAD = (9, 120, 250)
# name -> (what decode() is asked for, the tensor canvas)
CASES = {
    "coded": (dict(), None),
    "crop": (dict(output="crop"), None),
    "box": (dict(output=(64, 48)), (64, 64)),
    "rotate": (dict(rotate=90), None),
    "color": (dict(color="bt709"), None),
}


@pytest.fixture(scope="module")
def stream():
    s, _ = gen.make_stream_crop(WMB, HMB, F, [CROP], seed=11, profile="high")
    return s


@pytest.fixture(scope="module")
def table():
    return R.value_table(SCALE, BIAS)


def _rgb(s, order, ask, **opts):
    """seq -> (rc, out_w, out_h, the RGB bytes) of an MVHP_OUT_RGB_ONLY call"""
    got = {}
    eng = Engine(**opts)

    def sink(seq, idr, rc, err, p, g, yuv, rgb):
        got[seq] = (rc, g.out_w, g.out_h, None if rgb is None else rgb.copy())
        return 1 if rc == 1 else 0

    try:
        rc, st = eng.decode(s.h, order, want_rgb=3, sink=sink, score=True, **ask)   # (score: the sink with the geometry, always)
    finally:
        eng.close()
    return rc, st, got


def _tensors(s, order, ask, canvas, dtype, layout, bgr, **opts):
    """seq -> (rc, err, the length the geometry carries, the tensor's bytes, whether planes came) of a host-delivered call"""
    got = {}
    eng = Engine(**opts)

    def sink(seq, idr, rc, err, p, g, yuv, t):
        got[seq] = (rc, err, g.reserved[0], None if t is None else t.copy(), yuv is not None)
        return 1 if rc == 1 else 0

    try:
        eng.set_tensor(canvas, dtype, layout, bgr, PAD, SCALE, BIAS)
        rc, st = eng.decode(s.h, order, sink=sink, tensor=True, **ask)
    finally:
        eng.close()
    return rc, st, got


@pytest.mark.parametrize("dtype,layout,bgr", [("float16", "nchw", False), ("float32", "nhwc", True), ("bfloat16", "nchw", True)])
@pytest.mark.parametrize("case", list(CASES))
def test_host_delivery_is_the_reference_of_the_rgb(stream, table, case, dtype, layout, bgr):
    ask, canvas = CASES[case]
    order = list(range(F)) + [2, 0]
    opts = dict(contexts=2, batch_pictures=3, chunk_pictures=2)
    with Stream(stream) as s:
        assert s.ok and s.idr_count == F
        rc0, st0, rgb = _rgb(s, order, ask, **opts)
        rc1, st1, ten = _tensors(s, order, ask, canvas, dtype, layout, bgr, **opts)
    assert rc0 == 1 and rc1 == 1 and st1["pictures_ok"] == len(order) and st1["pictures_failed"] == 0
    code, lay = H.TENSOR_DTYPES.index(dtype), H.TENSOR_LAYOUTS.index(layout)
    total = 0
    for seq in range(len(order)):
        ok, w, h, px = rgb[seq]
        assert ok == 1 and ten[seq][0] == 1 and not ten[seq][4]
        want = R.pack(px.reshape(1, h, w, 3), canvas, code, lay, bgr, PAD, table=table)[0]
        assert ten[seq][2] == want.size == R.tensor_bytes(w, h, canvas, code), (seq, ten[seq][2], want.size)
        assert ten[seq][3].tobytes() == want.tobytes(), (case, seq)
        total += want.size
    assert st1["d2h_bytes"] == total
    if case == "box":
        assert all(rgb[k][1] <= 64 and rgb[k][2] <= 48 for k in rgb)


def test_tensor_beside_the_score(stream, table):
    """MVHP_OUTPUT_SCORE composes: the same tensors, the score in g->reserved[1], 32 bytes more per picture"""
    order = list(range(F))
    scores, plain = {}, {}
    with Stream(stream) as s:
        for score, into in ((True, scores), (False, plain)):
            eng = Engine(contexts=1, batch_pictures=4)

            def sink(seq, idr, rc, err, p, g, yuv, t, into=into):
                into[seq] = (rc, g.score, g.reserved[0], t.tobytes())
                return 1

            try:
                eng.set_tensor(None, "float16", "nchw", False, PAD, SCALE, BIAS)
                rc, st = eng.decode(s.h, order, sink=sink, tensor=True, score=score)
            finally:
                eng.close()
            assert rc == 1
            into["d2h"] = st["d2h_bytes"]
    assert scores["d2h"] == plain["d2h"] + 32 * F
    assert all(scores[k][2:] == plain[k][2:] and plain[k][1] == 0 for k in range(F))
    assert all(scores[k][1] > 0 for k in range(F))


def test_device_delivery_equals_host_delivery(stream, table):
    torch = pytest.importorskip("torch")
    broken = _break_picture(stream, BROKEN)
    order = list(range(F)) + [1]
    for dtype, layout, bgr in (("float16", "nchw", False), ("float32", "nhwc", True)):
        with Stream(broken) as s:
            assert s.ok
            rc, st, ten = _tensors(s, order, dict(output=(64, 48)), (64, 64), dtype, layout, bgr, contexts=1, batch_pictures=3, chunk_pictures=2)
            eng = Engine(contexts=1, batch_pictures=3, chunk_pictures=2)
            try:
                out, ok = eng.decode_tensors(s.h, order, size=(64, 64), dtype=getattr(torch, dtype), layout=layout, mean=R.IMAGENET_MEAN,
                                             std=R.IMAGENET_STD, pad=PAD, bgr=bgr, output=(64, 48))
                again, ok2 = eng.decode_tensors(s.h, order, size=(64, 64), dtype=dtype, layout=layout, mean=R.IMAGENET_MEAN,
                                                std=R.IMAGENET_STD, pad=PAD, bgr=bgr, output=(64, 48))   # (the request is set anew)
            finally:
                eng.close()
        assert out.device.type == "cuda" and out.dtype == getattr(torch, dtype)
        assert tuple(out.shape) == ((len(order), 3, 64, 64) if layout == "nchw" else (len(order), 64, 64, 3))
        raw = out.cpu().contiguous().view(torch.uint8).numpy().reshape(len(order), -1)
        assert ok == ok2 == [seq != BROKEN for seq in range(len(order))]
        assert raw.tobytes() == again.cpu().contiguous().view(torch.uint8).numpy().tobytes()
        for seq in range(len(order)):
            if seq == BROKEN:
                assert ten[seq][0] != 1 and not raw[seq].any()                       # failed: its slot stays zero
            else:
                assert ten[seq][0] == 1 and raw[seq].tobytes() == ten[seq][3].tobytes(), seq


def test_over_range_pictures_leave_zeros(stream):
    """the cropped pictures are larger than a 64 x 64 canvas: every picture fails with a message, decoding goes on"""
    torch = pytest.importorskip("torch")
    order = list(range(F))
    ten = {}
    with Stream(stream) as s:
        eng = Engine(contexts=1)
        try:
            out, ok = eng.decode_tensors(s.h, order, size=(64, 64), output="crop")

            def sink(seq, idr, rc, err, p, g, yuv, t):
                ten[seq] = (rc, err, t)
                return 0

            eng.set_tensor((64, 64), "float16")
            eng.decode(s.h, order, sink=sink, tensor=True, output="crop")
        finally:
            eng.close()
    assert ok == [False] * F and not out.cpu().view(torch.uint8).numpy().any()
    assert all(ten[k][0] != 1 and "canvas" in ten[k][1] and ten[k][2] is None for k in range(F))


def test_pictures_past_the_target_fail_and_touch_nothing(stream, table):
    torch = pytest.importorskip("torch")
    order = list(range(F))
    tb = 3 * 64 * 64 * 2
    buf = torch.full((F * tb,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))
    seen = {}
    with Stream(stream) as s:
        rc0, st0, ten = _tensors(s, order, dict(output=(64, 48)), (64, 64), "float16", "nchw", False, contexts=1)
        eng = Engine(contexts=1, batch_pictures=2)

        def sink(seq, idr, rc, err, p, g, yuv, t):
            seen[seq] = (rc, err, g.reserved[0], yuv is None and t is None)
            return 1 if rc == 1 else 0

        try:
            torch.cuda.synchronize()
            eng.set_tensor((64, 64), "float16", "nchw", False, PAD, SCALE, BIAS, d_target=buf.data_ptr(), target_pictures=4)
            rc, st = eng.decode(s.h, order, sink=sink, tensor=True, output=(64, 48))
        finally:
            eng.close()
    raw = buf.cpu().numpy().reshape(F, tb)
    assert rc == 1 and st["d2h_bytes"] == 0 and st["pictures_ok"] == 4 and st["pictures_failed"] == F - 4
    for seq in range(F):
        assert seen[seq][3]
        if seq < 4:
            assert seen[seq][0] == 1 and seen[seq][2] == tb and raw[seq].tobytes() == ten[seq][3].tobytes()
        else:
            assert seen[seq][0] != 1 and "slots" in seen[seq][1] and (raw[seq] == 0xA5).all()


def _raw_decode(eng, s, order, mask, flags=0):
    arr = (C.c_int * len(order))(*order)
    req = H.OutputRequest(flags, 0, 0, 0)
    st = H.DecodeStats()
    return eng._L.mvhp_engine_decode_ex(eng._h, s.h, arr, len(order), len(order), mask, C.byref(req), C.cast(None, H.SINK_EX_T), None, C.byref(st)), st


def test_refusals(stream, monkeypatch):
    torch = pytest.importorskip("torch")
    buf = torch.zeros(F * 3 * 64 * 64 * 2, dtype=torch.uint8, device=torch.device("cuda", 0))
    with Stream(stream) as s:
        eng = Engine(contexts=1)
        try:
            rc, st = _raw_decode(eng, s, [0, 1], H.OUT_TENSOR)                            # no request set
            assert rc != 1 and st.batches == 0
            eng.set_tensor(None, "float16")
            assert _raw_decode(eng, s, [0, 1], H.OUT_TENSOR)[0] == 1
            for mask, flags in ((H.OUT_TENSOR | H.OUT_JPEG, 0), (H.OUT_TENSOR | H.OUT_PNG, 0), (H.OUT_TENSOR, H.OUTPUT_BARS)):
                rc, st = _raw_decode(eng, s, [0, 1], mask, flags)
                assert rc != 1 and st.batches == 0, (mask, flags)
            for kw in (dict(jpeg=80), dict(png=True), dict(bars=True)):
                with pytest.raises(ValueError):
                    eng.decode(s.h, [0], sink=lambda *a: 1, tensor=True, **kw)
            eng.set_tensor(clear=True)
            assert _raw_decode(eng, s, [0, 1], H.OUT_TENSOR)[0] != 1
            for bad in (dict(dtype=3), dict(layout=2), dict(canvas=(64, 0)), dict(canvas=(16385, 64)), dict(scale=(1.0, float("inf"), 1.0)),
                        dict(d_target=buf.data_ptr() + 8, target_pictures=2), dict(d_target=buf.data_ptr(), target_pictures=0)):
                with pytest.raises(H.MiniVideoError):
                    eng.set_tensor(**bad)
        finally:
            eng.close()
        monkeypatch.setenv("MINIVIDEO_FAKE_GPUS", "2")
        eng = Engine()
        try:
            assert eng.contexts == 2
            with pytest.raises(ValueError):
                eng.decode_tensors(s.h, [0, 1], size=(64, 64))
            eng.set_tensor((64, 64), "float16", d_target=buf.data_ptr(), target_pictures=F)
            rc, st = _raw_decode(eng, s, [0, 1], H.OUT_TENSOR)
            assert rc != 1 and st.batches == 0
            eng.set_tensor((128, 96), "float16")                                          # host delivery runs on any engine
            assert _raw_decode(eng, s, [0, 1], H.OUT_TENSOR)[0] == 1
        finally:
            eng.close()
    assert not buf.cpu().numpy().any()
