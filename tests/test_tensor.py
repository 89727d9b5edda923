"""Tensor output, the parts that need no device: the NumPy restatement (tests/tensor_ref.py) against float64 mathematics, and the
two host functions of the C-ABI, mvhp_tensor_constants and mvhp_tensor_bytes."""
import numpy as np
import pytest

from minivideo_amd import hotpath as H
from tests import tensor_ref as R


def _ulp(v):
    v = np.float32(abs(v))
    return float(np.nextafter(v, np.float32(np.inf))) - float(v)


def test_reference_against_float64_within_one_ulp():
    """all 256 x 3 entries for the ImageNet constants: the exactly rounded fused multiply-add is within one binary32 ulp of the
    float64 evaluation (which is itself off by far less than that), and within half an ulp of it almost everywhere"""
    scale, bias = R.constants(R.IMAGENET_MEAN, R.IMAGENET_STD)
    tab = R.value_table(scale, bias)
    assert tab.shape == (256, 3) and tab.dtype == np.float32
    for k in range(3):
        for c in range(256):
            want = float(c) * float(scale[k]) + float(bias[k])
            assert abs(float(tab[c, k]) - want) <= _ulp(want), (c, k, tab[c, k], want)


def test_reference_rounding_rules():
    """ties to even, subnormals, overflow and the sign of zero, on values chosen for them"""
    one, eps = np.float32(1.0), np.float32(2.0 ** -24)
    assert R.fma_f32(1, one, eps) == np.float32(1.0)                                  # 1 + 2^-24: a tie, the even neighbour is 1
    assert R.fma_f32(3, eps, one) == np.float32(1.0 + 2.0 ** -22)                     # 1 + 3 * 2^-24: a tie, up to the even one
    assert R.fma_f32(1, np.float32(2.0 ** -149), 0.0).view(np.uint32) == 1            # the smallest subnormal is kept
    assert R.fma_f32(255, np.float32(3e38), np.float32(3e38)) == np.float32(np.inf)
    assert R.fma_f32(255, np.float32(-3e38), np.float32(-3e38)) == np.float32(-np.inf)
    assert not np.signbit(R.fma_f32(0, np.float32(-1.0), np.float32(0.0)))            # -0 + +0
    assert np.signbit(R.fma_f32(0, np.float32(-1.0), np.float32(-0.0)))               # -0 + -0
    assert not np.signbit(R.fma_f32(5, np.float32(1.0), np.float32(-5.0)))            # exact cancellation
    # a product that float32 could not hold on its own: one rounding, not two (255 * (1 + 2^-23) - 255 = 255 * 2^-23 exactly)
    assert R.fma_f32(255, np.float32(1.0 + 2.0 ** -23), np.float32(-255.0)) == np.float32(255 * 2.0 ** -23)
    bf = R.to_bf16_bits(np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, np.inf, 2.0 ** -133], np.float32))
    assert list(bf) == [0x3f80, 0x3f80, 0x3f82, 0x7f80, 0x0001]


@pytest.mark.parametrize("mean,std", [(R.IMAGENET_MEAN, R.IMAGENET_STD), ((0, 0, 0), (1, 1, 1)), ((0.5, 0.25, 0.125), (-0.5, 3.0, 1e-3)),
                                      ((127.5 / 255,) * 3, (1 / 255,) * 3)])
def test_constants_equal_the_double_computation_bit_for_bit(mean, std):
    scale, bias = H.tensor_constants(mean, std)
    ws, wb = R.constants(mean, std)
    assert scale.dtype == np.float32 and bias.dtype == np.float32
    assert scale.tobytes() == ws.tobytes() and bias.tobytes() == wb.tobytes()


@pytest.mark.parametrize("mean,std", [((0, 0, 0), (1, 0, 1)), ((0, 0, 0), (1, 1, float("nan"))), ((float("inf"), 0, 0), (1, 1, 1)),
                                      ((0, 0, 0), (float("inf"), 1, 1))])
def test_constants_refuse_zero_std_and_non_finite_input(mean, std):
    with pytest.raises(ValueError):
        H.tensor_constants(mean, std)


def test_tensor_bytes_for_every_dtype_and_layout():
    for dtype, es in ((H.TENSOR_F32, 4), (H.TENSOR_F16, 2), (H.TENSOR_BF16, 2)):
        for layout in (H.TENSOR_NCHW, H.TENSOR_NHWC):
            for bgr in (False, True):
                assert H.tensor_bytes(H.tensor_params(6, 4, None, dtype, layout, bgr)) == 3 * 6 * 4 * es
                assert H.tensor_bytes(H.tensor_params(6, 4, (7, 5), dtype, layout, bgr)) == 3 * 7 * 5 * es
                assert H.tensor_bytes(H.tensor_params(130, 66, (224, 224), dtype, layout, bgr)) == 3 * 224 * 224 * es
                assert H.tensor_bytes(H.tensor_params(1, 1, (16384, 16384), dtype, layout, bgr)) == 3 * 16384 * 16384 * es
    assert H.tensor_bytes(H.tensor_params(16384, 16384, None, "float32")) == 3 * 16384 * 16384 * 4
    assert H.tensor_bytes(H.tensor_params(2, 2, None, "bfloat16", "nhwc")) == 24
    assert int(H.lib().mvhp_tensor_bytes(None)) == 0


def _bad(**kw):
    t = H.tensor_params(6, 4, (8, 8))
    for k, v in kw.items():
        setattr(t, k, v)
    return t


@pytest.mark.parametrize("kw", [dict(dtype=3), dict(dtype=0xffffffff), dict(layout=2), dict(flags=2), dict(flags=0x80000001),
                                dict(src_w=0), dict(src_h=0), dict(src_w=16385, canvas_w=0, canvas_h=0),
                                dict(src_h=16385, canvas_w=0, canvas_h=0), dict(canvas_w=16385), dict(canvas_h=16385),
                                dict(canvas_w=5), dict(canvas_h=3), dict(canvas_w=0), dict(canvas_h=0)])
def test_tensor_bytes_is_zero_for_each_bad_parameter(kw):
    assert H.tensor_bytes(_bad()) == 3 * 8 * 8 * 4
    assert H.tensor_bytes(_bad(**kw)) == 0


def test_reference_placement_layouts_and_channel_order():
    """a 2 x 1 picture on a 5 x 2 canvas: floor-divided offsets, pad colour per channel, NCHW planes, NHWC interleave, B,G,R"""
    rgb = np.array([[[[10, 20, 30], [40, 50, 60]]]], np.uint8)
    got = R.pack(rgb, (5, 2), R.F32, R.NHWC, pad=(1, 2, 3)).view(np.float32).reshape(2, 5, 3)
    assert got[0, 1].tolist() == [10, 20, 30] and got[0, 2].tolist() == [40, 50, 60]      # ox = 1, oy = 0
    assert got[0, 0].tolist() == [1, 2, 3] and (got[1] == [1, 2, 3]).all() and got[0, 3].tolist() == [1, 2, 3]
    planes = R.pack(rgb, (5, 2), R.F32, R.NCHW, bgr=True, pad=(1, 2, 3)).view(np.float32).reshape(3, 2, 5)
    assert planes[0, 0].tolist() == [3, 30, 60, 3, 3] and planes[2, 0].tolist() == [1, 10, 40, 1, 1]
    half = R.pack(rgb, None, R.F16, R.NCHW, scale=(2000,) * 3).view(np.float16).reshape(3, 1, 2)
    assert half[0, 0, 0] == np.float16(20000) and np.isinf(half[2, 0, 1])                 # 120000 is beyond binary16
