"""ctypes binding of include/minivideo_hotpath.h (the hot-path C-ABI)."""
import ctypes as C
import os

import numpy as np

SUCCESS, FAILURE, UNSUPPORTED = 1, 0, -1
STREAM_SPEC, STREAM_DEBLOCK = 1, 2                                     # mvhp_stream_open_ex flags (MVHP_STREAM_*)
PARAM_MAY_HAVE_8X8, PARAM_SPEC_LUMA_DC, PARAM_SLICES, PARAM_SCALING, PARAM_DEBLOCK = 1, 2, 4, 8, 16   # MVHP_PARAM_*
STAGE_RECON, STAGE_COLOR, STAGE_DEBLOCK = 1, 2, 4                      # mvhp_recon_stages_dev (MVHP_STAGE_*)
MB_BYTES = 800
MB_HEADER_BYTES = 32
# MVHP_RECON_ALIGN (= mvhp_recon_align()): alignment of d_packed / d_yuv / d_rgb of recon_dev and recon_stages_dev and of
# d_compact / d_packed of expand_compact_dev; a pointer below it is refused before anything is launched
RECON_ALIGN = 16

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


LAYOUTS = ("auto", "rows", "quad", "oct", "wide", "quad_wide", "pipe", "pipe1")   # MVHP_LAYOUT_*


class MiniVideoError(RuntimeError):
    pass


class StreamParams(C.Structure):
    """mvhp_stream_params_t"""
    _fields_ = [
        ("width_mbs", C.c_uint32),
        ("height_mbs", C.c_uint32),
        ("chroma_qp_index_offset", C.c_int32),
        ("second_chroma_qp_index_offset", C.c_int32),
        ("flags", C.c_uint32),
        ("scaling4", (C.c_uint8 * 16) * 3),   # MVHP_PARAM_SCALING: weight matrices, raster order (Intra Y, Cb, Cr)
        ("scaling8", C.c_uint8 * 64),         # ... Intra Y 8x8
    ]

    @property
    def mbs(self):
        return int(self.width_mbs) * int(self.height_mbs)

    @property
    def packed_bytes(self):
        return self.mbs * MB_BYTES

    @property
    def yuv_bytes(self):
        return self.mbs * 384

    @property
    def rgb_bytes(self):
        return self.mbs * 768


OUT_JPEG = 4                                                            # mvhp_engine_decode_ex output kind (MVHP_OUT_JPEG)
OUT_PNG = 8                                                             # ... (MVHP_OUT_PNG)
OUT_TENSOR = 16                                                         # ... (MVHP_OUT_TENSOR; Engine.set_tensor())
OUTPUT_CROP, OUTPUT_BOX, OUTPUT_SCORE = 1, 2, 4                          # mvhp_output_request_t flags (MVHP_OUTPUT_*)
OUTPUT_ORIENT, OUTPUT_ROTATE_SHIFT = 8, 4                                # ... the stream's own rotation; bits 4-5: further turns
OUTPUT_ASPECT, OUTPUT_COLOR, OUTPUT_COLOR_MODE_SHIFT = 0x800, 0x80, 8     # ... square samples; RGB by a colour pass, bits 8-10: its mode
MATRIX_BT601, MATRIX_BT709 = 0, 1                                       # mvhp_color_params_t::matrix (MVHP_MATRIX_*)
CHROMA_NEAREST, CHROMA_LEFT, CHROMA_CENTER = 0, 1, 2                    # mvhp_color_params_t::siting (MVHP_CHROMA_*)
COLOR_MODES = ("auto", "bt601", "bt709", "bt601-full", "bt709-full")    # MVHP_OUTPUT_COLOR_MODE(index); MINIVIDEO_COLOR's values
OUTPUT_BARS, OUTPUT_TRIM, BARS_LEVEL_SHIFT = 0x1000, 0x2000, 24           # ... probe the black bars (level in reserved bits 24-31); trim them
OUTPUT_HIST = 0x4000                                                    # ... count the plane histograms (Engine.picture_hist())
BARS_LEVEL_DEFAULT = 24                                                 # MVHP_BARS_LEVEL_DEFAULT
ORIENT_SRC_CODED = 1                                                    # mvhp_orient_dev src_flags (MVHP_ORIENT_SRC_CODED)


def rotate_flags(rotate):
    """None -> 0; "auto" -> MVHP_OUTPUT_ORIENT; 0 / 90 / 180 / 270 -> MVHP_OUTPUT_ROTATE(quarter turns); ("auto", angle) -> both:
    the angle on top of the stream's own rotation"""
    if rotate is None:
        return 0
    if isinstance(rotate, tuple):
        return rotate_flags(rotate[0]) | rotate_flags(rotate[1])
    if rotate == "auto":
        return OUTPUT_ORIENT
    if rotate not in (0, 90, 180, 270):
        raise ValueError('rotate must be "auto", 0, 90, 180 or 270')
    return (int(rotate) // 90) << OUTPUT_ROTATE_SHIFT


class OutputGeometry(C.Structure):
    """mvhp_output_geometry_t: the luma crop rectangle of the coded picture and the output size"""
    _fields_ = [("crop_x", C.c_uint32), ("crop_y", C.c_uint32), ("crop_w", C.c_uint32), ("crop_h", C.c_uint32),
                ("out_w", C.c_uint32), ("out_h", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    @property
    def yuv_bytes(self):
        return int(self.out_w) * int(self.out_h) * 3 // 2

    @property
    def rgb_bytes(self):
        return int(self.out_w) * int(self.out_h) * 3

    @property
    def score(self):
        """the picture's score (Engine.decode(score=True): MVHP_OUTPUT_SCORE), else 0"""
        return int(self.reserved[1])

    @property
    def bars(self):
        """the picture's content box (x, y, w, h) in coded coordinates (Engine.decode(bars=...): MVHP_OUTPUT_BARS); w = h = 0: none"""
        a, b = int(self.reserved[0]), int(self.reserved[1])
        return a & 0xffff, a >> 16, b & 0xffff, b >> 16


class OutputRequest(C.Structure):
    """mvhp_output_request_t"""
    _fields_ = [("flags", C.c_uint32), ("box_w", C.c_uint32), ("box_h", C.c_uint32), ("reserved", C.c_uint32)]


def color_flags(color):
    """None -> 0; one of COLOR_MODES -> MVHP_OUTPUT_COLOR | MVHP_OUTPUT_COLOR_MODE(its index)"""
    if color is None:
        return 0
    if color not in COLOR_MODES:
        raise ValueError("color must be one of " + ", ".join(COLOR_MODES))
    return OUTPUT_COLOR | (COLOR_MODES.index(color) << OUTPUT_COLOR_MODE_SHIFT)


def output_request(output, rotate=None, aspect=False, color=None, trim=False):
    """None -> None (the coded size); "crop" -> the SPS crop; (w, h) -> the crop fitted into a w x h box.  rotate (see
    rotate_flags()) adds the orientation bits; with rotate given the result is never None.  aspect=True adds
    MVHP_OUTPUT_ASPECT (square samples; implies the crop), color (see color_flags()) the colour bits; with either the result is
    never None.  trim=True adds MVHP_OUTPUT_TRIM (the stream's content box, stream_set_trim(); implies the crop)"""
    rot = rotate_flags(rotate) | (OUTPUT_ASPECT if aspect else 0) | color_flags(color) | (OUTPUT_TRIM if trim else 0)
    if output is None:
        return OutputRequest(rot, 0, 0, 0) if (rotate is not None or aspect or color is not None or trim) else None
    if output == "crop":
        return OutputRequest(OUTPUT_CROP | rot, 0, 0, 0)
    w, h = output
    return OutputRequest(OUTPUT_CROP | OUTPUT_BOX | rot, int(w), int(h), 0)


class JpegParams(C.Structure):
    """mvhp_jpeg_params_t"""
    _fields_ = [("quality", C.c_int32), ("restart_mcus", C.c_uint32), ("reserved", C.c_uint32)]


class JpegEntry(C.Structure):
    """mvhp_jpeg_entry_t: where a picture's file lies in the blob"""
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint32), ("status", C.c_uint32)]


JPEG_OK, JPEG_TOO_BIG = 0, 1                                            # mvhp_jpeg_entry_t status (MVHP_JPEG_*)
JPEG_STAGE_DCT, JPEG_STAGE_COUNT, JPEG_STAGE_WRITE = 1, 2, 4            # measurements only (MVHP_JPEG_STAGE_*)
JPEG_ENTRY_DTYPE = np.dtype([("offset", "<u8"), ("length", "<u4"), ("status", "<u4")])


def jpeg_header_bytes():
    return int(lib().mvhp_jpeg_header_bytes())


def jpeg_quant_tables(quality):
    """mvhp_jpeg_quant_tables: (2, 64) uint8, luma and chroma, row-major (no device needed)"""
    out = np.empty(128, dtype=np.uint8)
    if lib().mvhp_jpeg_quant_tables(int(quality), out.ctypes.data) != SUCCESS:
        raise MiniVideoError("mvhp_jpeg_quant_tables failed")
    return out.reshape(2, 64)


class PngParams(C.Structure):
    """mvhp_png_params_t"""
    _fields_ = [("reserved", C.c_uint32)]


PNG_OK, PNG_TOO_BIG = 0, 1                                              # mvhp_png_entry_t status (MVHP_PNG_*)
PNG_STAGE_ANALYSE, PNG_STAGE_PLACE, PNG_STAGE_WRITE = 1, 2, 4           # measurements only (MVHP_PNG_STAGE_*)
PNG_ENTRY_DTYPE = JPEG_ENTRY_DTYPE                                      # mvhp_png_entry_t: the table of both encoders
PNG_MAX_WIDTH = 21844                                                   # MVHP_PNG_MAX_WIDTH


def png_header_bytes():
    return int(lib().mvhp_png_header_bytes())


def png_segment_rows(w):
    """mvhp_png_segment_rows: rows per segment (= per IDAT chunk) of pictures w wide (no device needed)"""
    return int(lib().mvhp_png_segment_rows(int(w)))


def png_max_bytes(w, h):
    """mvhp_png_max_bytes: the longest file a w x h picture can give (no device needed)"""
    return int(lib().mvhp_png_max_bytes(int(w), int(h)))


class LumaStats(C.Structure):
    """mvhp_luma_stats_t: sums over the luma samples of a picture's rectangle"""
    _fields_ = [("sum", C.c_uint64), ("sumsq", C.c_uint64), ("samples", C.c_uint32), ("reserved", C.c_uint32 * 3)]


LUMA_STATS_DTYPE = np.dtype([("sum", "<u8"), ("sumsq", "<u8"), ("samples", "<u4"), ("reserved", "<u4", (3,))])


def luma_score(stats):
    """mvhp_luma_score: the luma variance of a LumaStats record (or a (sum, sumsq, samples) triple) in sixteenths, an integer
    (no device needed)"""
    if not isinstance(stats, LumaStats):
        s, q, n = stats
        stats = LumaStats(int(s), int(q), int(n))
    return int(lib().mvhp_luma_score(C.byref(stats)))


def blank_choose(scores, min_score):
    """mvhp_blank_choose: index of the first score >= min_score, else of the largest (the earliest on a tie); -1 for none"""
    arr = (C.c_uint32 * max(len(scores), 1))(*[int(x) for x in scores])
    return int(lib().mvhp_blank_choose(arr, len(scores), int(min_score)))


class PlaneHist(C.Structure):
    """mvhp_plane_hist_t: the histograms of the three planes over a picture's rectangle"""
    _fields_ = [("y", C.c_uint32 * 256), ("cb", C.c_uint32 * 256), ("cr", C.c_uint32 * 256), ("samples", C.c_uint32),
                ("chroma_samples", C.c_uint32), ("reserved", C.c_uint32 * 6)]


PLANE_HIST_DTYPE = np.dtype([("y", "<u4", (256,)), ("cb", "<u4", (256,)), ("cr", "<u4", (256,)), ("samples", "<u4"),
                             ("chroma_samples", "<u4"), ("reserved", "<u4", (6,))])


def _hist_array(hists):
    """PLANE_HIST_DTYPE records (an array, one record, or raw bytes) -> a contiguous 1-D array of them"""
    if isinstance(hists, (bytes, bytearray, memoryview)):
        hists = np.frombuffer(hists, PLANE_HIST_DTYPE)
    a = np.ascontiguousarray(hists, dtype=PLANE_HIST_DTYPE).reshape(-1)
    return a


def hist_stats(hist):
    """mvhp_hist_stats: the LumaStats record of the rectangle a PLANE_HIST_DTYPE record was counted over (no device needed)"""
    a = _hist_array(hist)
    if a.size != 1:
        raise ValueError("hist_stats takes one record")
    out = LumaStats()
    if lib().mvhp_hist_stats(a.ctypes.data, C.byref(out)) != SUCCESS:
        raise MiniVideoError("mvhp_hist_stats failed")
    return out


def represent_choose(hists, eligible=None):
    """mvhp_represent_choose: the index of the candidate closest to the candidates' mean histogram (the earliest on a tie), -1
    for none; eligible: one flag per record, None = all (no device needed)"""
    a = _hist_array(hists)
    el = None
    if eligible is not None:
        if len(eligible) != a.size:
            raise ValueError("one eligibility flag per record")
        el = (C.c_uint8 * max(a.size, 1))(*[1 if x else 0 for x in eligible])
    return int(lib().mvhp_represent_choose(a.ctypes.data if a.size else None, int(a.size), el))


TENSOR_F32, TENSOR_F16, TENSOR_BF16 = 0, 1, 2                           # mvhp_tensor_params_t::dtype (MVHP_TENSOR_*)
TENSOR_NCHW, TENSOR_NHWC = 0, 1                                         # ... ::layout
TENSOR_BGR = 1                                                          # ... ::flags
TENSOR_DTYPES = ("float32", "float16", "bfloat16")
TENSOR_LAYOUTS = ("nchw", "nhwc")


class TensorParams(C.Structure):
    """mvhp_tensor_params_t: dense RGB8 pictures of src_w x src_h -> tensors of canvas_h x canvas_w (0, 0 = the picture's size)"""
    _fields_ = [("src_w", C.c_uint32), ("src_h", C.c_uint32), ("canvas_w", C.c_uint32), ("canvas_h", C.c_uint32),
                ("dtype", C.c_uint32), ("layout", C.c_uint32), ("flags", C.c_uint32), ("pad_rgb", C.c_uint32),
                ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


class TensorRequest(C.Structure):
    """mvhp_tensor_request_t: what Engine.set_tensor() hands to the MVHP_OUT_TENSOR calls that follow"""
    _fields_ = [("canvas_w", C.c_uint32), ("canvas_h", C.c_uint32), ("dtype", C.c_uint32), ("layout", C.c_uint32),
                ("flags", C.c_uint32), ("pad_rgb", C.c_uint32), ("scale", C.c_float * 3), ("bias", C.c_float * 3),
                ("d_target", C.c_void_p), ("target_pictures", C.c_uint32), ("reserved", C.c_uint32)]


def _tensor_code(value, names, what):
    if isinstance(value, int):
        return value
    name = str(value).replace("torch.", "").lower()
    if name not in names:
        raise ValueError("%s %r (one of %s)" % (what, value, ", ".join(names)))
    return names.index(name)


def tensor_params(src_w, src_h, canvas=None, dtype="float32", layout="nchw", bgr=False, pad=(0, 0, 0), scale=(1.0, 1.0, 1.0),
                  bias=(0.0, 0.0, 0.0)):
    """a TensorParams: canvas = (w, h) or None for the picture's size; dtype a name of TENSOR_DTYPES (or a torch dtype), layout
    a name of TENSOR_LAYOUTS; pad = the (r, g, b) of the canvas outside the picture; scale, bias per R, G, B"""
    t = TensorParams()
    t.src_w, t.src_h = int(src_w), int(src_h)
    t.canvas_w, t.canvas_h = (int(canvas[0]), int(canvas[1])) if canvas else (0, 0)
    t.dtype = _tensor_code(dtype, TENSOR_DTYPES, "tensor dtype")
    t.layout = _tensor_code(layout, TENSOR_LAYOUTS, "tensor layout")
    t.flags = TENSOR_BGR if bgr else 0
    t.pad_rgb = (int(pad[0]) & 255) << 16 | (int(pad[1]) & 255) << 8 | (int(pad[2]) & 255)
    for k in range(3):
        t.scale[k], t.bias[k] = scale[k], bias[k]
    return t


def tensor_bytes(params):
    """mvhp_tensor_bytes: bytes of one picture's tensor, 0 for malformed parameters (no device needed)"""
    return int(lib().mvhp_tensor_bytes(C.byref(params)))


def tensor_constants(mean, std):
    """mvhp_tensor_constants: (scale, bias), two float32 arrays of three, for (x / 255 - mean) / std per R, G, B (no device
    needed); ValueError for std == 0 or non-finite input"""
    m, s = (C.c_double * 3)(*[float(x) for x in mean]), (C.c_double * 3)(*[float(x) for x in std])
    scale, bias = (C.c_float * 3)(), (C.c_float * 3)()
    if lib().mvhp_tensor_constants(m, s, scale, bias) != SUCCESS:
        raise ValueError("tensor_constants: std must not be 0 and mean, std must be finite")
    return np.array(scale[:], np.float32), np.array(bias[:], np.float32)


class LumaBars(C.Structure):
    """mvhp_luma_bars_t: the box of the content rows and columns of a picture's rectangle, coded coordinates"""
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("rows", C.c_uint32),
                ("cols", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    def as_tuple(self):
        return int(self.x), int(self.y), int(self.w), int(self.h), int(self.rows), int(self.cols)


LUMA_BARS_DTYPE = np.dtype([("x", "<u4"), ("y", "<u4"), ("w", "<u4"), ("h", "<u4"), ("rows", "<u4"), ("cols", "<u4"),
                            ("reserved", "<u4", (2,))])


def _as_bars(b):
    if b is None or isinstance(b, LumaBars):
        return b
    t = tuple(int(v) for v in b)
    return LumaBars(*t[:4]) if len(t) == 4 else LumaBars(*t[:6])


def bars_need(length):
    """mvhp_bars_need: bright samples that make a row of `length` samples (a column of `length` rows) content (no device needed)"""
    return int(lib().mvhp_bars_need(int(length)))


def bars_union(boxes):
    """mvhp_bars_union over LumaBars records or (x, y, w, h) tuples: (number of non-empty boxes, LumaBars of their union)"""
    recs = [_as_bars(b) for b in boxes]
    arr = (LumaBars * max(len(recs), 1))(*recs)
    out = LumaBars()
    n = int(lib().mvhp_bars_union(arr, len(recs), C.byref(out)))
    return n, out


def trim_rect(crop, union):
    """mvhp_trim_rect: (accepted 0 / 1, OutputGeometry) for the OutputGeometry `crop` and the LumaBars or (x, y, w, h) `union`"""
    out = OutputGeometry()
    u = _as_bars(union)
    rc = int(lib().mvhp_trim_rect(C.byref(crop), C.byref(u) if u is not None else None, C.byref(out)))
    return rc, out


def stream_set_trim(stream_handle, union):
    """mvhp_stream_set_trim: the stream carries the box (a LumaBars or (x, y, w, h)); None or an empty box clears it"""
    u = _as_bars(union)
    if lib().mvhp_stream_set_trim(stream_handle, C.byref(u) if u is not None else None) != SUCCESS:
        raise MiniVideoError("mvhp_stream_set_trim failed")


def stream_trim(stream_handle):
    """mvhp_stream_trim: the box the stream carries as (x, y, w, h); w = h = 0: none"""
    out = LumaBars()
    if lib().mvhp_stream_trim(stream_handle, C.byref(out)) != SUCCESS:
        raise MiniVideoError("mvhp_stream_trim failed")
    return out.as_tuple()[:4]


set_trim, trim = stream_set_trim, stream_trim   # (the stream-level pair under the library's verbs)


def geometry(crop_x, crop_y, crop_w, crop_h, out_w=None, out_h=None):
    g = OutputGeometry()
    g.crop_x, g.crop_y, g.crop_w, g.crop_h = crop_x, crop_y, crop_w, crop_h
    g.out_w, g.out_h = crop_w if out_w is None else out_w, crop_h if out_h is None else out_h
    return g


def geometry_fit(cw, ch, bw, bh):
    """the size rule (mvhp_geometry_fit): (out_w, out_h), or None for malformed arguments"""
    L = lib()
    ow, oh = C.c_uint32(), C.c_uint32()
    if L.mvhp_geometry_fit(cw, ch, bw, bh, C.byref(ow), C.byref(oh)) != SUCCESS:
        return None
    return ow.value, oh.value


def stream_crop(stream_handle, idr):
    """mvhp_stream_crop: OutputGeometry of the SPS crop of picture `idr`, or None (mvhp_stream_last_error() says why)"""
    g = OutputGeometry()
    return g if lib().mvhp_stream_crop(stream_handle, int(idr), C.byref(g)) == SUCCESS else None


def stream_rotation(stream_handle):
    """mvhp_stream_rotation: the display rotation of an MP4's video track, clockwise, 0 / 90 / 180 / 270 (Annex B: 0)"""
    return int(lib().mvhp_stream_rotation(stream_handle))


def output_turns(stream_handle, output=None, rotate=None):
    """mvhp_output_turns: the quarter turns (0 .. 3) output_request(output, rotate) applies to pictures of the stream"""
    req = output_request(output, rotate)
    return int(lib().mvhp_output_turns(stream_handle, C.byref(req) if req is not None else None))


class DisplayInfo(C.Structure):
    """mvhp_display_info_t: what the VUI of a picture's SPS says about display"""
    _fields_ = [("sar_w", C.c_uint32), ("sar_h", C.c_uint32), ("vui_present", C.c_uint32), ("signal_present", C.c_uint32),
                ("full_range", C.c_uint32), ("matrix_coefficients", C.c_uint32), ("chroma_loc", C.c_uint32),
                ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class ColorParams(C.Structure):
    """mvhp_color_params_t"""
    _fields_ = [("matrix", C.c_int32), ("full_range", C.c_int32), ("siting", C.c_int32), ("reserved", C.c_int32)]

    def as_tuple(self):
        return int(self.matrix), int(self.full_range), int(self.siting)


def stream_display(stream_handle, idr):
    """mvhp_stream_display: DisplayInfo of picture `idr` (sample aspect ratio, range, matrix, chroma location), or None"""
    d = DisplayInfo()
    return d if lib().mvhp_stream_display(stream_handle, int(idr), C.byref(d)) == SUCCESS else None


def color_coefficients(matrix, full_range):
    """mvhp_color_coefficients: (cy, crv, cbu, gcb, gcr, yoff), or None for values the header does not name (no device needed)"""
    out = (C.c_int32 * 6)()
    if lib().mvhp_color_coefficients(int(matrix), int(full_range), out) != SUCCESS:
        return None
    return tuple(int(x) for x in out)


def color_resolve(display, coded_w, coded_h, mode=0):
    """mvhp_color_resolve: ColorParams for pictures of coded_w x coded_h whose stream says `display` (a DisplayInfo or None) under
    `mode` (0 .. 4 or one of COLOR_MODES), or None for a mode outside them (no device needed)"""
    if isinstance(mode, str):
        mode = COLOR_MODES.index(mode)
    out = ColorParams()
    rc = lib().mvhp_color_resolve(C.byref(display) if display is not None else None, int(coded_w), int(coded_h), int(mode), C.byref(out))
    return out if rc == SUCCESS else None


def geometry_aspect(cw, ch, sar_w, sar_h):
    """the aspect rule (mvhp_geometry_aspect): (out_w, out_h), or None for malformed arguments"""
    ow, oh = C.c_uint32(), C.c_uint32()
    if lib().mvhp_geometry_aspect(cw, ch, sar_w, sar_h, C.byref(ow), C.byref(oh)) != SUCCESS:
        return None
    return ow.value, oh.value


def output_geometry(stream_handle, idr, output, rotate=None, aspect=False, trim=False):
    """mvhp_output_geometry under output_request(output, rotate, aspect, trim=trim), or None: what the sink gets"""
    g = OutputGeometry()
    req = output_request(output, rotate, aspect, trim=trim)
    rc = lib().mvhp_output_geometry(stream_handle, int(idr), C.byref(req) if req is not None else None, C.byref(g))
    return g if rc == SUCCESS else None


class PlanDevice(C.Structure):
    """mvhp_plan_device_t: what the launch planner needs to know of a device, and the forced settings (0 = choose)"""
    _fields_ = [("n_cus", C.c_int32), ("max_lds_bytes", C.c_uint64), ("layout", C.c_int32), ("waves", C.c_int32)]


def plan_launch(dev, params, n_frames):
    """mvhp_plan_launch for a described device (no GPU needed): (layout name, waves per workgroup) a launch of n_frames
    pictures would run on, or None for malformed arguments"""
    lay, nw = C.c_int(0), C.c_int(0)
    if lib().mvhp_plan_launch(None, C.byref(dev), C.byref(params), int(n_frames), C.byref(lay), C.byref(nw)) != SUCCESS:
        return None
    return LAYOUTS[lay.value], nw.value


def lib_path():
    # MINIVIDEO_LIB: developer override used for A/B experiments with alternative builds of the same library
    return os.environ.get("MINIVIDEO_LIB") or os.path.join(_HERE, "libminivideo.so")


def lib():
    """Load libminivideo.so (in-tree build). Fails loudly when it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise MiniVideoError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no pure-Python or CPU fallback for the reconstruction path)")
    L = C.CDLL(path, mode=C.RTLD_GLOBAL)
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    pp = C.POINTER(StreamParams)
    L.mvhp_last_error.restype = C.c_char_p
    for f in ("mvhp_packed_frame_bytes", "mvhp_yuv_frame_bytes", "mvhp_rgb_frame_bytes"):
        getattr(L, f).restype = sz
        getattr(L, f).argtypes = [pp]
    L.mvhp_device_count.restype = i32
    L.mvhp_create.restype = i32
    L.mvhp_create.argtypes = [i32, C.POINTER(vp)]
    L.mvhp_destroy.restype = None
    L.mvhp_destroy.argtypes = [vp]
    L.mvhp_set_waves_per_picture.restype = i32
    L.mvhp_set_waves_per_picture.argtypes = [vp, i32]
    L.mvhp_set_layout.restype = i32
    L.mvhp_set_layout.argtypes = [vp, i32]
    L.mvhp_set_fused_color.restype = i32
    L.mvhp_set_fused_color.argtypes = [vp, i32]
    L.mvhp_set_crop_copy.restype = i32
    L.mvhp_set_crop_copy.argtypes = [vp, i32]
    L.mvhp_recon_align.restype = sz
    L.mvhp_recon_align.argtypes = []
    L.mvhp_recon_batch_dev.restype = i32
    L.mvhp_recon_batch_dev.argtypes = [vp, pp, vp, i32, vp, vp, vp]
    L.mvhp_expand_compact_dev.restype = i32
    L.mvhp_expand_compact_dev.argtypes = [vp, pp, vp, sz, i32, vp, vp]
    L.mvhp_recon_stages_dev.restype = i32
    L.mvhp_recon_stages_dev.argtypes = [vp, pp, vp, i32, vp, vp, vp, i32]
    L.mvhp_recon_batch_host.restype = i32
    L.mvhp_recon_batch_host.argtypes = [vp, pp, vp, i32, vp, vp]
    L.mvhp_sync_check.restype = i32
    L.mvhp_sync_check.argtypes = [vp, vp]
    L.mvhp_last_launch_info.restype = i32
    L.mvhp_last_launch_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.mvhp_debug_set_wide_state.restype = i32
    L.mvhp_debug_set_wide_state.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.mvhp_debug_get_wide_state.restype = i32
    L.mvhp_debug_get_wide_state.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(sz)]
    L.mvhp_plan_launch.restype = i32
    L.mvhp_plan_launch.argtypes = [vp, C.POINTER(PlanDevice), pp, i32, C.POINTER(i32), C.POINTER(i32)]
    pg, u32 = C.POINTER(OutputGeometry), C.c_uint32
    L.mvhp_stream_crop.restype = i32
    L.mvhp_stream_crop.argtypes = [vp, i32, pg]
    L.mvhp_output_geometry.restype = i32
    L.mvhp_output_geometry.argtypes = [vp, i32, C.POINTER(OutputRequest), pg]
    L.mvhp_geometry_fit.restype = i32
    L.mvhp_geometry_fit.argtypes = [u32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32)]
    for f in ("mvhp_geometry_yuv_bytes", "mvhp_geometry_rgb_bytes"):
        getattr(L, f).restype = sz
        getattr(L, f).argtypes = [pg]
    L.mvhp_resample_dev.restype = i32
    L.mvhp_resample_dev.argtypes = [vp, pp, pg, vp, i32, vp, vp, vp]
    L.mvhp_orient_dev.restype = i32
    L.mvhp_orient_dev.argtypes = [vp, pp, pg, i32, u32, vp, i32, vp, vp, vp]
    L.mvhp_stream_display.restype = i32
    L.mvhp_stream_display.argtypes = [vp, i32, C.POINTER(DisplayInfo)]
    L.mvhp_geometry_aspect.restype = i32
    L.mvhp_geometry_aspect.argtypes = [u32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32)]
    L.mvhp_color_coefficients.restype = i32
    L.mvhp_color_coefficients.argtypes = [i32, i32, C.POINTER(C.c_int32)]
    L.mvhp_color_resolve.restype = i32
    L.mvhp_color_resolve.argtypes = [C.POINTER(DisplayInfo), u32, u32, i32, C.POINTER(ColorParams)]
    L.mvhp_color_dev.restype = i32
    L.mvhp_color_dev.argtypes = [vp, pg, C.POINTER(ColorParams), vp, i32, vp, vp]
    L.mvhp_stream_rotation.restype = i32
    L.mvhp_stream_rotation.argtypes = [vp]
    L.mvhp_output_turns.restype = i32
    L.mvhp_output_turns.argtypes = [vp, C.POINTER(OutputRequest)]
    L.mvhp_luma_score.restype = C.c_uint32
    L.mvhp_luma_score.argtypes = [C.POINTER(LumaStats)]
    L.mvhp_blank_choose.restype = i32
    L.mvhp_blank_choose.argtypes = [C.POINTER(C.c_uint32), i32, C.c_uint32]
    L.mvhp_luma_stats_dev.restype = i32
    L.mvhp_luma_stats_dev.argtypes = [vp, pp, pg, vp, i32, vp, vp]
    L.mvhp_set_stats_band.restype = i32
    L.mvhp_set_stats_band.argtypes = [vp, i32]
    L.mvhp_hist_stats.restype = i32
    L.mvhp_hist_stats.argtypes = [vp, C.POINTER(LumaStats)]
    L.mvhp_represent_choose.restype = i32
    L.mvhp_represent_choose.argtypes = [vp, i32, vp]
    L.mvhp_plane_hist_dev.restype = i32
    L.mvhp_plane_hist_dev.argtypes = [vp, pp, pg, vp, i32, vp, vp]
    L.mvhp_set_hist_band.restype = i32
    L.mvhp_set_hist_band.argtypes = [vp, i32]
    L.mvhp_tensor_bytes.restype = sz
    L.mvhp_tensor_bytes.argtypes = [C.POINTER(TensorParams)]
    L.mvhp_tensor_constants.restype = i32
    L.mvhp_tensor_constants.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.mvhp_tensor_dev.restype = i32
    L.mvhp_tensor_dev.argtypes = [vp, C.POINTER(TensorParams), vp, i32, vp, vp, vp]
    L.mvhp_set_tensor_rows.restype = i32
    L.mvhp_set_tensor_rows.argtypes = [vp, i32]
    pb = C.POINTER(LumaBars)
    L.mvhp_bars_need.restype = u32
    L.mvhp_bars_need.argtypes = [u32]
    L.mvhp_bars_union.restype = i32
    L.mvhp_bars_union.argtypes = [pb, i32, pb]
    L.mvhp_trim_rect.restype = i32
    L.mvhp_trim_rect.argtypes = [pg, pb, pg]
    L.mvhp_stream_set_trim.restype = i32
    L.mvhp_stream_set_trim.argtypes = [vp, pb]
    L.mvhp_stream_trim.restype = i32
    L.mvhp_stream_trim.argtypes = [vp, pb]
    L.mvhp_luma_bars_dev.restype = i32
    L.mvhp_luma_bars_dev.argtypes = [vp, pp, pg, vp, i32, i32, vp, vp]
    L.mvhp_set_bars_band.restype = i32
    L.mvhp_set_bars_band.argtypes = [vp, i32]
    L.mvhp_jpeg_header_bytes.restype = sz
    L.mvhp_jpeg_header_bytes.argtypes = []
    L.mvhp_jpeg_quant_tables.restype = i32
    L.mvhp_jpeg_quant_tables.argtypes = [i32, vp]
    L.mvhp_jpeg_encode_dev.restype = i32
    L.mvhp_jpeg_encode_dev.argtypes = [vp, pg, C.POINTER(JpegParams), vp, i32, vp, sz, vp, vp]
    L.mvhp_png_header_bytes.restype = sz
    L.mvhp_png_header_bytes.argtypes = []
    L.mvhp_png_segment_rows.restype = i32
    L.mvhp_png_segment_rows.argtypes = [i32]
    L.mvhp_png_max_bytes.restype = sz
    L.mvhp_png_max_bytes.argtypes = [i32, i32]
    L.mvhp_png_encode_dev.restype = i32
    L.mvhp_png_encode_dev.argtypes = [vp, pg, C.POINTER(PngParams), vp, i32, vp, sz, vp, vp]
    L.mvhp_stream_last_error.restype = C.c_char_p
    if hasattr(L, "mvhp_stream_open"):
        L.mvhp_stream_open.restype = i32
        L.mvhp_stream_open.argtypes = [vp, sz, C.POINTER(vp)]
        L.mvhp_stream_close.restype = None
        L.mvhp_stream_close.argtypes = [vp]
        L.mvhp_stream_idr_count.restype = i32
        L.mvhp_stream_idr_count.argtypes = [vp]
        L.mvhp_stream_params.restype = i32
        L.mvhp_stream_params.argtypes = [vp, i32, pp]
        L.mvhp_stream_decode_packed.restype = i32
        L.mvhp_stream_decode_packed.argtypes = [vp, i32, vp, sz]
    _LIB = L
    return L


def _err(L, what):
    msg = L.mvhp_last_error()
    return MiniVideoError(f"{what}: {msg.decode() if msg else 'failed'}")


class HotPath:
    """One GPU reconstruction context (mvhp_ctx_t): device + stream + scratch."""

    def __init__(self, device=0):
        self._L = lib()
        h = C.c_void_p()
        if self._L.mvhp_create(int(device), C.byref(h)) != SUCCESS:
            raise _err(self._L, "mvhp_create")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._L.mvhp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_waves_per_picture(self, waves):
        if self._L.mvhp_set_waves_per_picture(self._h, int(waves)) != SUCCESS:
            raise MiniVideoError("waves per picture must be 0 (auto), 1, 2, 4, 6, 8, 12 or 16")

    def set_layout(self, layout):
        """A name of LAYOUTS or its index (MVHP_LAYOUT_*): 0 auto, 1 one picture per workgroup (rows), 2 four pictures per
        workgroup (quad), 3 eight (oct), 4 one picture over several workgroups (wide), 5 four pictures over several workgroups
        (quad_wide), 6 the same with three wavefronts per macroblock row (pipe), 7 one picture per wavefront, three wavefronts
        per row (pipe1); speed only.  A form that cannot run the batch (line buffers that do not fit in LDS, slices / scaling
        matrices) is replaced: plan_launch() says by which."""
        code = LAYOUTS.index(layout) if layout in LAYOUTS else layout
        if self._L.mvhp_set_layout(self._h, int(code)) != SUCCESS:
            raise ValueError("layout must be one of " + "/".join(LAYOUTS))

    def set_fused_color(self, on):
        self._L.mvhp_set_fused_color(self._h, 1 if on else 0)

    def set_crop_copy(self, on):
        """True (default): crop-only geometries run the copy kernel; False: the general resample kernel.  Speed only."""
        self._L.mvhp_set_crop_copy(self._h, 1 if on else 0)

    # -- host buffers ------------------------------------------------------
    def recon_host(self, params, packed, n_frames, want_rgb=False):
        """packed: uint8 array of n_frames*params.packed_bytes -> (yuv, rgb|None) uint8 arrays."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8).reshape(-1)
        if packed.size != n_frames * params.packed_bytes:
            raise ValueError("packed buffer size does not match params/n_frames")
        yuv = np.empty(n_frames * params.yuv_bytes, dtype=np.uint8)
        rgb = np.empty(n_frames * params.rgb_bytes, dtype=np.uint8) if want_rgb else None
        rc = self._L.mvhp_recon_batch_host(
            self._h, C.byref(params), packed.ctypes.data, int(n_frames), yuv.ctypes.data,
            rgb.ctypes.data if want_rgb else None)
        if rc != SUCCESS:
            raise _err(self._L, "mvhp_recon_batch_host")
        return yuv, rgb

    # -- device pointers (e.g. torch tensors' data_ptr()) --------------------
    def recon_dev(self, params, d_packed, n_frames, d_yuv, d_rgb=None, stream=None):
        rc = self._L.mvhp_recon_batch_dev(self._h, C.byref(params), d_packed, int(n_frames), d_yuv, d_rgb, stream)
        if rc != SUCCESS:
            raise _err(self._L, "mvhp_recon_batch_dev")

    def expand_compact_dev(self, params, d_compact, stride, n_pictures, d_packed, stream=None):
        """compact pictures (transfer format) -> packed records, both in device memory"""
        rc = self._L.mvhp_expand_compact_dev(self._h, C.byref(params), d_compact, int(stride), int(n_pictures), d_packed, stream)
        if rc != SUCCESS:
            raise _err(self._L, "mvhp_expand_compact_dev")

    def recon_stages_dev(self, params, d_packed, n_frames, d_yuv, d_rgb, stream, stages):
        rc = self._L.mvhp_recon_stages_dev(self._h, C.byref(params), d_packed, int(n_frames), d_yuv, d_rgb,
                                           stream, int(stages))
        if rc != SUCCESS:
            raise _err(self._L, "mvhp_recon_stages_dev")

    def resample_dev(self, params, geom, d_yuv_coded, n, d_yuv_out=None, d_rgb_out=None, stream=None):
        """n coded pictures (device) -> n pictures of OutputGeometry `geom`: planes and / or RGB (device)"""
        rc = self._L.mvhp_resample_dev(self._h, C.byref(params), C.byref(geom), d_yuv_coded, int(n), d_yuv_out, d_rgb_out, stream)
        if rc != SUCCESS:
            raise _err(self._L, "mvhp_resample_dev")

    def orient_dev(self, params, geom, quarter_turns, d_src, n, d_yuv_out=None, d_rgb_out=None, coded=True, stream=None):
        """n pictures (device) turned by quarter_turns (0 .. 3, clockwise) into planes and / or RGB (device).  geom is the
        geometry BEFORE the turn; coded=True: d_src holds coded pictures of `params` and geom's crop rectangle is read out of
        them (out size = crop size); coded=False: d_src holds dense pictures of geom.out_w x geom.out_h (params may be None).
        Output pictures are out_h x out_w for odd turns.  Asynchronous."""
        rc = self._L.mvhp_orient_dev(self._h, C.byref(params) if params is not None else None, C.byref(geom), int(quarter_turns),
                                     ORIENT_SRC_CODED if coded else 0, d_src, int(n), d_yuv_out, d_rgb_out, stream)
        if rc != SUCCESS:
            raise _err(self._L, "mvhp_orient_dev")

    def color_dev(self, geom, color, d_yuv, n, d_rgb_out, stream=None):
        """n dense planar pictures of geom.out_w x geom.out_h (device) -> n RGB pictures (device) by `color`, a ColorParams or a
        (matrix, full_range, siting) triple.  Asynchronous."""
        if not isinstance(color, ColorParams):
            color = ColorParams(int(color[0]), int(color[1]), int(color[2]), 0)
        rc = self._L.mvhp_color_dev(self._h, C.byref(geom), C.byref(color), d_yuv, int(n), d_rgb_out, stream)
        if rc != SUCCESS:
            raise _err(self._L, "mvhp_color_dev")

    def luma_stats_dev(self, params, geom, d_yuv_coded, n, d_stats, stream=None):
        """n coded pictures (device) -> n LumaStats records (LUMA_STATS_DTYPE, device) over geom's crop rectangle.  Asynchronous."""
        rc = self._L.mvhp_luma_stats_dev(self._h, C.byref(params), C.byref(geom), d_yuv_coded, int(n), d_stats, stream)
        if rc != SUCCESS:
            raise _err(self._L, "mvhp_luma_stats_dev")

    def plane_hist_dev(self, params, geom, d_yuv_coded, n, d_hist, stream=None):
        """n coded pictures (device) -> n PlaneHist records (PLANE_HIST_DTYPE, device, 16-byte aligned): the luma histogram over
        geom's crop rectangle, Cb and Cr over the same rectangle halved.  Asynchronous."""
        rc = self._L.mvhp_plane_hist_dev(self._h, C.byref(params), C.byref(geom), d_yuv_coded, int(n), d_hist, stream)
        if rc != SUCCESS:
            raise _err(self._L, "mvhp_plane_hist_dev")

    def tensor_dev(self, params, d_rgb, n, d_out, slots=None, stream=None):
        """n dense RGB8 pictures (device, 4-byte aligned) -> n tensors of tensor_bytes(params) at d_out (device, 16-byte aligned):
        picture i in slot slots[i] (a device pointer to n int32; negative = skipped), or in slot i.  Asynchronous."""
        rc = self._L.mvhp_tensor_dev(self._h, C.byref(params) if params is not None else None, d_rgb, int(n), d_out, slots, stream)
        if rc != SUCCESS:
            raise _err(self._L, "mvhp_tensor_dev")

    def set_tensor_rows(self, rows):
        """test-only: canvas rows per workgroup of tensor_dev, 0 = choose (speed only: the tensors do not depend on it)"""
        if self._L.mvhp_set_tensor_rows(self._h, int(rows)) != SUCCESS:
            raise MiniVideoError("mvhp_set_tensor_rows(%d) failed" % rows)

    def set_hist_band(self, rows):
        """test-only: luma rows per workgroup of plane_hist_dev, 0 = choose (speed only: the records do not depend on it)"""
        if self._L.mvhp_set_hist_band(self._h, int(rows)) != SUCCESS:
            raise MiniVideoError("mvhp_set_hist_band(%d) failed" % rows)

    def luma_bars_dev(self, params, geom, d_yuv_coded, n, level, d_bars, stream=None):
        """n coded pictures (device) -> n LumaBars records (LUMA_BARS_DTYPE, device) over geom's crop rectangle: a sample is bright
        when it is above `level` (1 .. 254).  Asynchronous."""
        rc = self._L.mvhp_luma_bars_dev(self._h, C.byref(params), C.byref(geom), d_yuv_coded, int(n), int(level), d_bars, stream)
        if rc != SUCCESS:
            raise _err(self._L, "mvhp_luma_bars_dev")

    def set_bars_band(self, rows):
        """test-only: luma rows per workgroup of luma_bars_dev's counting pass, 0 = choose (speed only: the records do not depend on it)"""
        if self._L.mvhp_set_bars_band(self._h, int(rows)) != SUCCESS:
            raise MiniVideoError("mvhp_set_bars_band(%d) failed" % rows)

    def set_stats_band(self, rows):
        """test-only: luma rows per workgroup of luma_stats_dev, 0 = choose (speed only: the records do not depend on it)"""
        if self._L.mvhp_set_stats_band(self._h, int(rows)) != SUCCESS:
            raise MiniVideoError("mvhp_set_stats_band(%d) failed" % rows)

    def png_encode_dev(self, geom, d_rgb, n, d_blob, cap_bytes, d_table, stream=None, stages=0):
        """n pictures of OutputGeometry `geom` (dense RGB8, device) -> PNG files in d_blob (16-byte aligned, cap_bytes) and n
        records (PNG_ENTRY_DTYPE) in d_table, both device memory.  Asynchronous.  stages: measurements only (PNG_STAGE_*), 0 = the
        whole encode."""
        pp = PngParams(int(stages))
        rc = self._L.mvhp_png_encode_dev(self._h, C.byref(geom), C.byref(pp), d_rgb, int(n), d_blob, int(cap_bytes), d_table, stream)
        if rc != SUCCESS:
            raise _err(self._L, "mvhp_png_encode_dev")

    def jpeg_encode_dev(self, geom, d_yuv, n, d_blob, cap_bytes, d_table, quality=75, restart_mcus=0, stream=None, stages=0):
        """n pictures of OutputGeometry `geom` (planar, device) -> JPEG files in d_blob (16-byte aligned, cap_bytes) and n
        JpegEntry records (JPEG_ENTRY_DTYPE) in d_table, both device memory; restart_mcus 0 = one MCU row.  Asynchronous.
        stages: measurements only (JPEG_STAGE_*), 0 = the whole encode."""
        jp = JpegParams(int(quality), int(restart_mcus), int(stages))
        rc = self._L.mvhp_jpeg_encode_dev(self._h, C.byref(geom), C.byref(jp), d_yuv, int(n), d_blob, int(cap_bytes), d_table, stream)
        if rc != SUCCESS:
            raise _err(self._L, "mvhp_jpeg_encode_dev")

    def sync_check(self, stream=None):
        if self._L.mvhp_sync_check(self._h, stream) != SUCCESS:
            raise _err(self._L, "mvhp_sync_check")

    def set_wide_state(self, ticket, epoch):
        """test hook (mvhp_debug_set_wide_state): the ticket counter of the banded forms, on the device and in the host's
        bookkeeping, and the epoch tag of the last banded launch; waits for every launch issued on the context first"""
        if self._L.mvhp_debug_set_wide_state(self._h, int(ticket), int(epoch)) != SUCCESS:
            raise _err(self._L, "mvhp_debug_set_wide_state")

    def get_wide_state(self):
        """test hook (mvhp_debug_get_wide_state): (ticket counter on the device, the host's mirror of it, epoch tag of the
        last banded launch, bytes of the seam buffer), once every launch issued on the context has run"""
        dev, base, epoch, seam = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_size_t()
        if self._L.mvhp_debug_get_wide_state(self._h, C.byref(dev), C.byref(base), C.byref(epoch), C.byref(seam)) != SUCCESS:
            raise _err(self._L, "mvhp_debug_get_wide_state")
        return dev.value, base.value, epoch.value, seam.value

    def plan_launch(self, params, n_frames):
        """(layout name, waves per workgroup) the next reconstruction launch of n_frames pictures would use on this context"""
        lay, nw = C.c_int(0), C.c_int(0)
        if self._L.mvhp_plan_launch(self._h, None, C.byref(params), int(n_frames), C.byref(lay), C.byref(nw)) != SUCCESS:
            raise MiniVideoError("mvhp_plan_launch: invalid argument")
        return LAYOUTS[lay.value], nw.value

    def last_launch(self):
        """(layout name, waves per workgroup) of the last reconstruction launch -- speed-only choices of the launcher."""
        lay, nw = C.c_int(0), C.c_int(0)
        self._L.mvhp_last_launch_info(self._h, C.byref(lay), C.byref(nw))
        return (LAYOUTS[lay.value] if 0 <= lay.value < len(LAYOUTS) else "?"), nw.value


# ---------------------------------------------------------------------------
# placed batch buffers (mvhp_placed_alloc): records, planes and RGB each in a group of the memory system of its own
# ---------------------------------------------------------------------------
class PlacedBuffers:
    """Device buffers of the given sizes inside one large allocation, each -- as far as the device shows several groups of
    memory regions -- in a group of its own (DESIGN.md 3 "Placement"; the fastest placement of a batch's three streams).
    .ptrs: device addresses; .groups: group index per buffer (-1 = straddles); .groups_found; .seconds.  close() frees all."""

    def __init__(self, device, sizes, arena_bytes=0):
        import time
        L = lib()
        L.mvhp_placed_alloc.restype = C.c_int
        L.mvhp_placed_alloc.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mvhp_placed_free.restype = None
        L.mvhp_placed_free.argtypes = [C.c_void_p]
        n = len(sizes)
        arr, ptrs, arena = (C.c_size_t * n)(*[int(v) for v in sizes]), (C.c_void_p * n)(), C.c_void_p()
        gof, gf = (C.c_int * n)(), C.c_int()
        t0 = time.perf_counter()
        if L.mvhp_placed_alloc(int(device), n, arr, int(arena_bytes), ptrs, C.byref(arena), gof, C.byref(gf)) != SUCCESS:
            raise MiniVideoError("mvhp_placed_alloc: not enough free device memory for the arena (use ordinary allocations)")
        self.seconds = time.perf_counter() - t0
        self._L, self._arena = L, arena
        self.ptrs = [int(p) for p in ptrs]
        self.groups = [int(g) for g in gof]
        self.groups_found = int(gf.value)

    def close(self):
        if getattr(self, "_arena", None):
            self._L.mvhp_placed_free(self._arena)
            self._arena = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------
# decode engine (mvhp_engine_*): stream bytes -> reconstructed pictures, pipelined
# ---------------------------------------------------------------------------
class EngineOpts(C.Structure):
    """mvhp_engine_opts_t"""
    _fields_ = [("contexts", C.c_int32), ("host_threads", C.c_int32), ("batch_pictures", C.c_int32),
                ("chunk_pictures", C.c_int32), ("fail_context", C.c_int32), ("first_device", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class DecodeStats(C.Structure):
    """mvhp_decode_stats_t"""
    _fields_ = [("pictures_issued", C.c_uint32), ("pictures_ok", C.c_uint32), ("pictures_failed", C.c_uint32),
                ("batches", C.c_uint32), ("batches_requeued", C.c_uint32), ("contexts", C.c_uint32),
                ("host_threads", C.c_uint32), ("launches_by_layout", C.c_uint32 * 4), ("max_batch_pictures", C.c_uint32),
                ("wall_s", C.c_double), ("entropy_busy_s", C.c_double), ("h2d_s", C.c_double), ("kernel_s", C.c_double),
                ("d2h_s", C.c_double), ("sink_s", C.c_double), ("stream_bytes", C.c_uint64), ("h2d_bytes", C.c_uint64),
                ("d2h_bytes", C.c_uint64), ("host_alloc_s", C.c_double), ("dev_alloc_s", C.c_double),
                ("first_launch_s", C.c_double), ("first_picture_s", C.c_double), ("host_alloc_bytes", C.c_uint64),
                ("dev_alloc_bytes", C.c_uint64), ("placed_buffers", C.c_uint32), ("geometry_launches", C.c_uint32),
                ("launches_wide", C.c_uint32 * 4)]

    def as_dict(self):
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = list(v) if hasattr(v, "__len__") else v
        return d


SINK_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(StreamParams),
                     C.POINTER(C.c_uint8), C.POINTER(C.c_uint8))


SINK_EX_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(StreamParams),
                        C.POINTER(OutputGeometry), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8))


class Engine:
    """mvhp_engine_t: host entropy threads -> H2D -> batched kernels -> D2H -> sink, over every context."""

    def __init__(self, contexts=0, host_threads=0, batch_pictures=0, chunk_pictures=0, fail_context=-1, first_device=0, placed=False):
        self._L = L = lib()
        L.mvhp_engine_create.restype = C.c_int
        L.mvhp_engine_create.argtypes = [C.POINTER(EngineOpts), C.POINTER(C.c_void_p)]
        L.mvhp_engine_destroy.restype = None
        L.mvhp_engine_destroy.argtypes = [C.c_void_p]
        L.mvhp_engine_decode.restype = C.c_int
        L.mvhp_engine_decode.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, SINK_T,
                                         C.c_void_p, C.POINTER(DecodeStats)]
        L.mvhp_engine_decode_ex.restype = C.c_int
        L.mvhp_engine_decode_ex.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                            C.POINTER(OutputRequest), SINK_EX_T, C.c_void_p, C.POINTER(DecodeStats)]
        L.mvhp_engine_release_picture.restype = None
        L.mvhp_engine_release_picture.argtypes = [C.c_void_p, C.c_int]
        L.mvhp_engine_picture_hist.restype = C.c_void_p
        L.mvhp_engine_picture_hist.argtypes = [C.c_void_p, C.c_int]
        L.mvhp_engine_contexts.restype = C.c_int
        L.mvhp_engine_contexts.argtypes = [C.c_void_p]
        self._device = int(first_device)
        L.mvhp_engine_set_tensor.restype = C.c_int
        L.mvhp_engine_set_tensor.argtypes = [C.c_void_p, C.POINTER(TensorRequest)]
        o = EngineOpts(contexts, host_threads, batch_pictures, chunk_pictures, fail_context, first_device)
        o.reserved[0] = 1 if placed else 0   # bit 0: batch buffers from mvhp_placed_alloc_sets (same as MINIVIDEO_PLACED=1)
        h = C.c_void_p()
        if L.mvhp_engine_create(C.byref(o), C.byref(h)) != SUCCESS:
            raise MiniVideoError("mvhp_engine_create failed (no HIP device? there is no CPU reconstruction path)")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.mvhp_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def release_picture(self, seq):
        """gives back a picture whose sink call answered 2 (any thread; the decode call returns when the last one is back)"""
        self._L.mvhp_engine_release_picture(self._h, int(seq))

    def picture_hist(self, seq):
        """mvhp_engine_picture_hist: the PLANE_HIST_DTYPE record (a copy, shape ()) of picture `seq` of a decode(hist=True) call,
        for use inside the sink call for `seq` (or for a kept picture until its release); None for a failed picture, without
        hist=True and at any other time"""
        p = self._L.mvhp_engine_picture_hist(self._h, int(seq))
        if not p:
            return None
        return np.frombuffer(C.string_at(p, PLANE_HIST_DTYPE.itemsize), PLANE_HIST_DTYPE)[0].copy()

    def set_tensor(self, canvas=None, dtype="float32", layout="nchw", bgr=False, pad=(0, 0, 0), scale=(1.0, 1.0, 1.0),
                   bias=(0.0, 0.0, 0.0), d_target=None, target_pictures=0, clear=False):
        """mvhp_engine_set_tensor: the tensors of the decode(tensor=True) calls that follow (the arguments of tensor_params();
        canvas None = every tensor has its picture's size).  d_target = a device pointer to target_pictures tensors (16-byte
        aligned): device delivery, picture seq straight into slot seq, on an engine of one context.  clear=True takes the
        request back.  MiniVideoError for a request the library refuses."""
        if clear:
            self._L.mvhp_engine_set_tensor(self._h, None)
            return
        t = tensor_params(1, 1, None, dtype, layout, bgr, pad, scale, bias)
        r = TensorRequest()
        r.canvas_w, r.canvas_h = (int(canvas[0]), int(canvas[1])) if canvas else (0, 0)
        r.dtype, r.layout, r.flags, r.pad_rgb = t.dtype, t.layout, t.flags, t.pad_rgb
        for k in range(3):
            r.scale[k], r.bias[k] = t.scale[k], t.bias[k]
        r.d_target, r.target_pictures = d_target, int(target_pictures)
        if self._L.mvhp_engine_set_tensor(self._h, C.byref(r)) != SUCCESS:
            raise MiniVideoError("mvhp_engine_set_tensor refused the request (see the message on stderr)")

    @property
    def contexts(self):
        """mvhp_engine_contexts: the number of device contexts the engine runs"""
        return int(self._L.mvhp_engine_contexts(self._h))

    def decode_tensors(self, stream_handle, order, size=None, dtype=None, layout="nchw", mean=(0, 0, 0), std=(1, 1, 1), pad=(0, 0, 0),
                       bgr=False, output=None, rotate=None, aspect=False, color=None, trim=False):
        """The pictures order[...] as one normalised batch tensor that never leaves the device -> (tensor, ok).
        tensor: a torch.Tensor on the engine's device, [len(order), 3, h, w] (layout "nchw") or [len(order), h, w, 3] ("nhwc"), of
        dtype torch.float16 (the default), torch.float32 or torch.bfloat16 (or their names): (x / 255 - mean) / std per R, G, B
        (bgr=True: channel order B, G, R), under the contract of mvhp_tensor_dev.  size = (w, h): every picture is fitted into
        that box (output=None: the box is `size`; pictures are never enlarged) and centred on a canvas of that size filled with
        `pad` = (r, g, b); size=None: the tensor has the pictures' own size, which must be one size.  output, rotate, aspect,
        color and trim are decode()'s.  ok: one boolean per picture; the slot of a picture that failed (or does not fit) is zero.
        Device delivery: ValueError on an engine of more than one context."""
        import torch
        if self.contexts != 1:
            raise ValueError("decode_tensors writes into one device's memory: the engine must have exactly one context (has %d)" % self.contexts)
        code = _tensor_code(dtype if dtype is not None else "float16", TENSOR_DTYPES, "tensor dtype")
        lay = _tensor_code(layout, TENSOR_LAYOUTS, "tensor layout")
        if size is not None and output is None:
            output = (int(size[0]), int(size[1]))
        if size is not None:
            w, h = int(size[0]), int(size[1])
        else:
            g = output_geometry(stream_handle, order[0], output, rotate, aspect, trim) if len(order) else None
            if g is None:
                raise ValueError("decode_tensors without a size: the first picture has no geometry to take it from")
            w, h = g.out_w, g.out_h
        n = len(order)
        shape = (n, 3, h, w) if lay == TENSOR_NCHW else (n, h, w, 3)
        out = torch.zeros(shape, dtype=getattr(torch, TENSOR_DTYPES[code]), device=torch.device("cuda", self._device))
        ok = [False] * n
        scale, bias = tensor_constants(mean, std)

        def sink(seq, idr, rc, err, p, g, yuv, rgb):
            ok[seq] = rc == SUCCESS
            return 1 if rc == SUCCESS else 0

        torch.cuda.synchronize(out.device)   # (the zeros are there before the engine's own queue writes over them)
        self.set_tensor((w, h) if size is not None else None, code, lay, bgr, pad, scale, bias, d_target=out.data_ptr(), target_pictures=n)
        try:
            if n:
                self.decode(stream_handle, order, sink=sink, output=output, rotate=rotate, aspect=aspect, color=color, trim=trim, tensor=True)
        finally:
            self.set_tensor(clear=True)
        return out, ok

    def decode(self, stream_handle, order, wanted=None, want_rgb=False, sink=None, output=None, jpeg=None, restart_mcus=0,
               score=False, rotate=None, png=False, aspect=False, color=None, bars=None, trim=False, hist=False, tensor=False):
        """sink(seq, idr, rc, err, params, yuv ndarray | None, rgb ndarray | None) -> 1 accept / 0 reject / -1 stop /
        2 accept and keep until release_picture(seq); the arrays are views of page-locked memory valid only during the call
        (or until the release).  Returns (rc, stats dict).
        output (see output_request()): None = pictures of the coded size (mvhp_engine_decode); "crop" or a (w, h) box =
        mvhp_engine_decode_ex, and the sink is called with one more argument after params, the picture's OutputGeometry (a
        copy): sink(seq, idr, rc, err, params, geometry, yuv, rgb), the arrays sized by it.
        jpeg = a quality (1 .. 100): MVHP_OUT_JPEG -- the pictures (of the coded size, or of `output`) are coded as JPEG on the
        device and only the files come back: sink(seq, idr, rc, err, params, geometry, None, file bytes as a uint8 array);
        want_rgb is ignored; restart_mcus 0 = one MCU row.
        png=True: MVHP_OUT_PNG -- the pictures' RGB is coded as PNG on the device and only the files come back, handed to the sink
        as the JPEG files are; not together with jpeg.
        score=True: MVHP_OUTPUT_SCORE -- the sink is called as for `output` (with the geometry, also for pictures of the coded
        size) and finds each picture's score in geometry.score; the pictures are the same bytes.
        rotate = "auto" (the stream's own rotation, stream_rotation()) or 0 / 90 / 180 / 270 (clockwise): the pictures are
        turned on the device; the sink is called as for `output`, and its geometry is the one of the turned picture.
        aspect=True: MVHP_OUTPUT_ASPECT -- the stream's sample aspect ratio is applied (square samples out); implies the crop.
        color = "auto" or "bt601" / "bt709" / "bt601-full" / "bt709-full": MVHP_OUTPUT_COLOR -- the RGB (and the PNG files) are
        made from the final planes by the stream's own matrix, range and chroma siting, or by the forced matrix and range.
        bars = True (level 24) or a level 1 .. 254: MVHP_OUTPUT_BARS -- the sink is called as for `output` and finds each picture's
        content box in geometry.bars; the pictures are the same bytes.  Not together with jpeg, png or score, and it needs a
        sink (ValueError).
        trim=True: MVHP_OUTPUT_TRIM -- the crop of every picture is trimmed to the box the stream carries (stream_set_trim())
        where the trim rule accepts it; implies the crop.
        hist=True: MVHP_OUTPUT_HIST -- the sink is called as for `output` and reads its picture's plane histograms with
        picture_hist(seq); the pictures are the same bytes.  Not together with bars.
        tensor=True: MVHP_OUT_TENSOR -- the RGB `output`, rotate, aspect, color and trim deliver is packed into the tensors of
        set_tensor() on the device and only those come back: sink(seq, idr, rc, err, params, geometry, None, the tensor's bytes
        as a uint8 array) -- or, with set_tensor(d_target=...), nothing comes back and the last argument is None too.  Not
        together with jpeg, png or bars (ValueError)."""
        order = (C.c_int * len(order))(*order)
        st = DecodeStats()
        n_wanted = len(order) if wanted is None else wanted
        if png and jpeg is not None:
            raise ValueError("png and jpeg are two output kinds: a call delivers one")
        probe = bars is not None and bars is not False
        if tensor and (jpeg is not None or png or probe):
            raise ValueError("tensor, jpeg, png and bars all use the geometry word that carries a length: a call delivers one")
        if probe:
            level = BARS_LEVEL_DEFAULT if bars is True else int(bars)
            if not 1 <= level <= 254:
                raise ValueError("bars must be True or a level between 1 and 254")
            if jpeg is not None or png or score:
                raise ValueError("bars travels in the geometry words that carry the file length and the score: not together with jpeg, png or score")
            if sink is None:
                raise ValueError("bars needs a sink: the boxes are delivered with the geometry")
            if hist:
                raise ValueError("bars and hist are two probes: a call runs one")
        if output is not None or jpeg is not None or score or rotate is not None or png or aspect or color is not None or probe or trim or hist or tensor:
            req = output_request(output, rotate, aspect, color, trim=bool(trim)) or OutputRequest(0, 0, 0, 0)
            if score:
                req.flags |= OUTPUT_SCORE
            if hist:
                req.flags |= OUTPUT_HIST
            if probe:
                req.flags |= OUTPUT_BARS
                req.reserved = level << BARS_LEVEL_SHIFT
            if jpeg is not None:
                req.reserved = (min(max(int(jpeg), 1), 100) & 0xff) | ((int(restart_mcus) & 0xffff) << 8)

            def _cbx(user, seq, idr, rc, err, p, g, yuv, rgb):
                if sink is None:
                    return 1 if rc == SUCCESS else 0
                pr, geom = p.contents, OutputGeometry.from_buffer_copy(g.contents)
                y = np.ctypeslib.as_array(yuv, shape=(geom.yuv_bytes,)) if yuv else None
                r = np.ctypeslib.as_array(rgb, shape=(geom.reserved[0] if jpeg is not None or png or tensor else geom.rgb_bytes,)) if rgb else None
                return int(sink(seq, idr, rc, err.decode() if err else "", pr, geom, y, r))

            cbx = SINK_EX_T(_cbx) if sink is not None else C.cast(None, SINK_EX_T)
            rc = self._L.mvhp_engine_decode_ex(self._h, stream_handle, order, len(order), n_wanted,
                                               OUT_JPEG if jpeg is not None else OUT_PNG if png else OUT_TENSOR if tensor else int(want_rgb), C.byref(req), cbx, None, C.byref(st))
            return rc, st.as_dict()

        def _cb(user, seq, idr, rc, err, p, yuv, rgb):
            if sink is None:
                return 1 if rc == SUCCESS else 0
            pr = p.contents
            y = np.ctypeslib.as_array(yuv, shape=(pr.yuv_bytes,)) if yuv else None
            r = np.ctypeslib.as_array(rgb, shape=(pr.rgb_bytes,)) if rgb else None
            return int(sink(seq, idr, rc, err.decode() if err else "", pr, y, r))

        cb = SINK_T(_cb) if sink is not None else C.cast(None, SINK_T)
        rc = self._L.mvhp_engine_decode(self._h, stream_handle, order, len(order), len(order) if wanted is None else wanted,
                                        int(want_rgb), cb, None, C.byref(st))   # 0 planes, 1 planes + RGB, 3 RGB only
        return rc, st.as_dict()
