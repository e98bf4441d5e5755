"""ctypes binding of include/eu_hip.h and a host mirror of envutil's job surface."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

SPHERICAL, CYLINDRICAL, RECTILINEAR, STEREOGRAPHIC, FISHEYE, CUBEMAP, BIATAN6 = range(7)
BC_MIRROR, BC_PERIODIC, BC_REFLECT, BC_NATURAL, BC_CONSTANT, BC_ZEROPAD, BC_GUESS = range(7)
PROJECTION_NAMES = ["spherical", "cylindrical", "rectilinear", "stereographic",
                    "fisheye", "cubemap", "biatan6"]


class EuError(RuntimeError):
    pass


class Facet(C.Structure):
    """struct eu_facet"""
    _fields_ = [("projection", C.c_int32), ("nchannels", C.c_int32),
                ("hfov", C.c_double),
                ("width", C.c_int32), ("height", C.c_int32),
                ("window_width", C.c_int32), ("window_height", C.c_int32),
                ("window_x_offset", C.c_int32), ("window_y_offset", C.c_int32),
                ("yaw", C.c_double), ("pitch", C.c_double), ("roll", C.c_double),
                ("brighten", C.c_double), ("step", C.c_double),
                ("has_lcp", C.c_int32),
                ("a", C.c_double), ("b", C.c_double), ("c", C.c_double),
                ("h", C.c_double), ("v", C.c_double), ("s", C.c_double),
                ("shear_g", C.c_double), ("shear_t", C.c_double),
                ("tr_x", C.c_double), ("tr_y", C.c_double), ("tr_z", C.c_double),
                ("tp_y", C.c_double), ("tp_p", C.c_double), ("tp_r", C.c_double),
                ("mask_paint", C.c_int32)]


class Container(C.Structure):
    """struct eu_container"""
    _fields_ = [("shape", C.c_int64 * 2), ("left", C.c_int64 * 2),
                ("right", C.c_int64 * 2), ("core", C.c_int64 * 2)]


class Target(C.Structure):
    """struct eu_target"""
    _fields_ = [("projection", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("bands", C.c_int32),       # in what was the alignment gap in front of x0: size and offsets stay
                ("x0", C.c_double), ("x1", C.c_double), ("y0", C.c_double), ("y1", C.c_double),
                ("yaw", C.c_double), ("pitch", C.c_double), ("roll", C.c_double),
                ("nchannels", C.c_int32), ("ntaps", C.c_int32),
                ("taps", C.POINTER(C.c_float)),
                ("row_begin", C.c_int32), ("row_end", C.c_int32), ("stage", C.c_int32),
                ("crop_x0", C.c_int32), ("crop_y0", C.c_int32),
                ("crop_w", C.c_int32), ("crop_h", C.c_int32),
                ("out_format", C.c_int32),
                ("band_rows", C.c_int32), ("band_count", C.c_int32), ("band_index", C.c_int32),
                ("synopsis", C.c_int32), ("single", C.POINTER(Facet)),
                ("feather", C.c_double)]


class Rays(C.Structure):
    """struct eu_rays"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ninputs", C.c_int32),
                ("nchannels", C.c_int32), ("ntaps", C.c_int32),
                ("taps", C.POINTER(C.c_float)),
                ("rays", C.c_void_p), ("ray_row_stride_bytes", C.c_size_t),
                ("rays_on_device", C.c_int32)]


class View(C.Structure):
    """struct eu_view"""
    _fields_ = [("yaw", C.c_double), ("pitch", C.c_double), ("roll", C.c_double),
                ("x0", C.c_double), ("x1", C.c_double), ("y0", C.c_double), ("y1", C.c_double)]


ROW_FLOATS = 24     # floats per row-table entry (EU_ROW_FLOATS)
OUT_FLOAT, OUT_SRGBA8 = 0, 1
SYN_PANORAMA, SYN_HDR_MERGE, SYN_FEATHER, SYN_MULTIBAND = 0, 1, 2, 4       # (3 is not assigned)


def lib_path():
    # EU_HIP_LIB: another build of the library (build-time A/B experiments)
    return os.environ.get("EU_HIP_LIB") or os.path.join(HERE, "lib", "libeu_hip.so")


def build(force=False):
    """compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)"""
    if force:
        subprocess.check_call(["make", "-s", "-C", HERE, "clean"])
    subprocess.check_call(["make", "-s", "-j8", "-C", HERE])
    return lib_path()


_lib = None


def _share_hip_runtime():
    """A PyTorch-ROCm wheel carries its own libamdhip64 / libhsa-runtime64, and a
    process that ends up with two HIP runtimes sees no GPU in the second one.
    When torch is installed, load its runtime first (without importing torch):
    libeu_hip.so's NEEDED libamdhip64.so.7 then binds to the same copy, whichever
    of the two is imported first."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise EuError(f"{p} is missing: run envutil_amd.build() (hipcc, gfx950). "
                      "There is no fallback implementation.")
    _share_hip_runtime()
    L = C.CDLL(p)
    vp, i32, f64 = C.c_void_p, C.c_int, C.c_double
    L.eu_hip_last_error.restype = C.c_char_p
    L.eu_hip_get_step.restype = f64
    L.eu_hip_get_step.argtypes = [i32, i32, i32, f64]
    L.eu_hip_get_extent.argtypes = [i32, i32, i32, f64, vp]
    L.eu_hip_make_spread.argtypes = [i32, i32, C.c_float, C.c_float, C.c_float, vp, i32]
    L.eu_hip_cubemap_metrics.argtypes = [i32, f64, i32, i32, vp, vp, vp, vp]
    L.eu_hip_container_geometry.argtypes = [i32, i32, i32, C.c_int64, C.c_int64, vp]
    L.eu_hip_source_load.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    L.eu_hip_source_load_edited.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    L.eu_hip_source_load_samples.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    L.eu_hip_source_load_rgbe.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    L.eu_hip_source_load_ycbcr.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    L.eu_hip_ycbcr_floats.argtypes = [vp, i32, i32, i32, vp]
    L.eu_hip_source_reload.argtypes = [vp, vp, i32, vp]
    L.eu_hip_source_load_pixels.argtypes = [vp, vp, i32, i32, i32, i32, C.c_uint, vp]
    L.eu_hip_source_edge_distance.argtypes = [vp, vp, C.c_size_t, i32, vp]
    L.eu_hip_source_has_edges.argtypes = [vp]
    L.eu_hip_source_edge_device_ptr.argtypes = [vp, vp]
    L.eu_hip_facet_alpha_dev.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    L.eu_hip_facet_alpha_rows.argtypes = [i32, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, i32]
    L.eu_hip_source_adopt.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    L.eu_hip_source_alloc.argtypes = [vp, i32, i32, i32, vp]
    L.eu_hip_source_device_ptr.argtypes = [vp, vp, vp]
    L.eu_hip_source_download.argtypes = [vp, vp, C.c_size_t]
    L.eu_hip_source_info.argtypes = [vp, vp, vp]
    L.eu_hip_source_update_facet.argtypes = [vp, vp]
    L.eu_hip_source_release.argtypes = [vp]
    L.eu_hip_render.argtypes = [vp, vp, i32, vp, C.c_size_t, i32, vp]
    L.eu_hip_render_samples.argtypes = [vp, vp, i32, vp, vp, C.c_size_t, i32, vp]
    L.eu_hip_encode_samples.argtypes = [vp, C.c_size_t, i32, i32, i32, i32, vp, vp, C.c_size_t, i32, vp]
    L.eu_hip_render_rgbe.argtypes = [vp, vp, i32, vp, C.c_size_t, i32, vp]
    L.eu_hip_encode_rgbe.argtypes = [vp, C.c_size_t, i32, i32, i32, vp, C.c_size_t, i32, vp]
    L.eu_hip_encode_ycbcr.argtypes = [vp, C.c_size_t, i32, i32, i32, i32, vp, vp]
    L.eu_hip_render_ycbcr.argtypes = [vp, vp, i32, vp, vp]
    L.eu_hip_ycbcr_planes.argtypes = [vp, C.c_size_t, i32, i32, i32, vp]
    L.eu_hip_init_devices.argtypes = [vp, i32]
    L.eu_hip_render_devices.argtypes = [vp, vp, i32, vp, C.c_size_t, i32]
    L.eu_hip_device_strips.argtypes = [vp, vp, i32, vp, vp]
    L.eu_hip_render_timed.argtypes = [vp, vp, i32, vp, C.c_size_t, i32, vp]
    L.eu_hip_render_rays.argtypes = [vp, vp, vp, C.c_size_t, i32, vp]
    L.eu_hip_render_rays_timed.argtypes = [vp, vp, vp, C.c_size_t, i32, vp]
    L.eu_hip_render_views.argtypes = [vp, vp, i32, vp, vp, C.c_size_t, C.c_size_t, i32, vp]
    L.eu_hip_render_views_multi.argtypes = [vp, vp, i32, vp, i32, vp, C.c_size_t, C.c_size_t, i32, vp]
    L.eu_hip_render_layers.argtypes = [vp, vp, i32, vp, C.c_size_t, C.c_size_t, i32, vp]
    L.eu_hip_view_tables.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.eu_hip_layout_segments.argtypes = [vp, vp, i32, vp, i32, vp]
    L.eu_hip_blend_layers.argtypes = [vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, i32, i32, i32, i32, i32,
                                      i32, i32, vp, C.c_size_t, i32, vp]
    L.eu_hip_multiband_scratch_bytes.argtypes = [vp, i32]
    L.eu_hip_multiband_scratch_bytes.restype = C.c_size_t
    L.eu_hip_multiband_levels.argtypes = [i32, i32, i32, i32]
    L.eu_hip_band_rows.argtypes = [i32, i32, i32, i32]
    L.eu_hip_band_rows.restype = i32
    L.eu_hip_malloc.argtypes = [vp, C.c_size_t]
    L.eu_hip_free.argtypes = [vp]
    L.eu_hip_memcpy_d2h.argtypes = [vp, vp, C.c_size_t]
    L.eu_hip_memcpy_h2d.argtypes = [vp, vp, C.c_size_t]
    _lib = L
    return L


def _check(rc):
    if rc < 0:
        raise EuError(f"eu_hip error {rc}: {lib().eu_hip_last_error().decode()}")
    return rc


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def device_count():
    return lib().eu_hip_device_count()


def get_extent(projection, width, height, hfov):
    e = np.zeros(4, np.float64)
    _check(lib().eu_hip_get_extent(projection, width, height, hfov, _ptr(e)))
    return e


def get_step(projection, width, height, hfov):
    return lib().eu_hip_get_step(projection, width, height, hfov)


def make_spread(w, h=0, d=1.0, sigma=0.0, threshold=0.0):
    n = max(w, 2) * max(h if h > 0 else max(w, 2), 1)
    out = np.zeros((n, 3), np.float32)
    k = _check(lib().eu_hip_make_spread(w, h, d, sigma, threshold, _ptr(out), n))
    return out[:k].copy()


class MaskPolygon(C.Structure):
    _fields_ = [("n", C.c_int), ("x", C.c_void_p), ("y", C.c_void_p)]


def facet_alpha(pixels, polygons=(), crop=None, crop_kind=0):
    """eu_hip_facet_alpha: PTO exclude masks (list of (xs, ys) vertex arrays) and the lens crop
    (x0, x1, y0, y1; kind 1 rectangular, 2 elliptic) of a facet, multiplied into `pixels`
    ((h, w, 2|4) float32, in place). Host function: works without a device. Returns the alpha plane."""
    assert pixels.dtype == np.float32 and pixels.ndim == 3 and pixels.flags.c_contiguous
    h, w, nch = pixels.shape
    keep = [(np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)) for x, y in polygons]
    arr = (MaskPolygon * max(len(keep), 1))()
    for i, (x, y) in enumerate(keep):
        arr[i].n, arr[i].x, arr[i].y = len(x), x.ctypes.data, y.ctypes.data
    alpha = np.zeros((h, w), np.float32)
    c = crop if crop is not None else (0, 0, 0, 0)
    f = lib().eu_hip_facet_alpha
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    _check(f(_ptr(pixels), w, h, nch, C.cast(arr, C.c_void_p), len(keep), crop_kind if crop is not None else 0,
             c[0], c[1], c[2], c[3], _ptr(alpha)))
    return alpha


class FacetEdit(C.Structure):
    """struct eu_facet_edit"""
    _fields_ = [("polygons", C.c_void_p), ("npolygons", C.c_int32),
                ("crop_kind", C.c_int32), ("crop_x0", C.c_int32), ("crop_x1", C.c_int32),
                ("crop_y0", C.c_int32), ("crop_y1", C.c_int32),
                ("pixel_channels", C.c_int32), ("pixels_on_device", C.c_int32)]


def _facet_edit(polygons, crop, crop_kind, pixel_channels, on_device):
    """(eu_facet_edit, objects it points into) for masks as a list of (xs, ys) and a crop (x0, x1, y0, y1)"""
    keep = [(np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)) for x, y in polygons]
    arr = (MaskPolygon * max(len(keep), 1))()
    for i, (x, y) in enumerate(keep):
        arr[i].n, arr[i].x, arr[i].y = len(x), x.ctypes.data, y.ctypes.data
    e = FacetEdit()
    e.polygons, e.npolygons = C.cast(arr, C.c_void_p), len(keep)
    e.crop_kind = crop_kind if crop is not None else 0
    e.crop_x0, e.crop_x1, e.crop_y0, e.crop_y1 = crop if crop is not None else (0, 0, 0, 0)
    e.pixel_channels, e.pixels_on_device = pixel_channels, int(on_device)
    return e, (keep, arr)


class Samples(C.Structure):
    """struct eu_samples"""
    _fields_ = [("data", C.c_void_p), ("bits", C.c_int32), ("big_endian", C.c_int32),
                ("pixel_channels", C.c_int32), ("on_device", C.c_int32),
                ("colour_table", C.c_void_p), ("alpha_table", C.c_void_p)]


class Rgbe(C.Structure):
    """struct eu_rgbe"""
    _fields_ = [("data", C.c_void_p), ("on_device", C.c_int32), ("colour_table", C.c_void_p)]


class Ycbcr(C.Structure):
    """struct eu_ycbcr"""
    _fields_ = [("y", C.c_void_p), ("cb", C.c_void_p), ("cr", C.c_void_p),
                ("y_pitch", C.c_size_t), ("c_pitch", C.c_size_t),
                ("c_step", C.c_int32), ("sub_x", C.c_int32), ("sub_y", C.c_int32),
                ("bits", C.c_int32), ("on_device", C.c_int32),
                ("y_table", C.c_void_p), ("c_table", C.c_void_p),
                ("m_rv", C.c_float), ("m_gu", C.c_float), ("m_gv", C.c_float), ("m_bu", C.c_float)]


class YcbcrOut(C.Structure):
    """struct eu_ycbcr_out"""
    _fields_ = [("y", C.c_void_p), ("cb", C.c_void_p), ("cr", C.c_void_p),
                ("y_pitch", C.c_size_t), ("c_pitch", C.c_size_t),
                ("c_step", C.c_int32), ("sub_x", C.c_int32), ("sub_y", C.c_int32),
                ("bits", C.c_int32), ("shift", C.c_int32), ("on_device", C.c_int32),
                ("y_steps", C.c_void_p), ("c_steps", C.c_void_p),
                ("k_r", C.c_float), ("k_g", C.c_float), ("k_b", C.c_float), ("c_u", C.c_float), ("c_v", C.c_float)]


PX_FLOATS, PX_SAMPLES, PX_RGBE, PX_YCBCR = 0, 1, 2, 3
LOAD_EDGES = 1                # eu_hip_source_load_pixels: keep the distance plane (feathering to alpha edges)


class Pixels(C.Structure):
    """struct eu_pixels"""
    _fields_ = [("kind", C.c_int32), ("floats", C.c_void_p), ("pixel_channels", C.c_int32),
                ("on_device", C.c_int32), ("samples", C.c_void_p), ("rgbe", C.c_void_p),
                ("ycbcr", C.c_void_p), ("edit", C.c_void_p)]


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def _settle(t, wait=True):
    """the work queued on a device tensor's current stream is done (wait=False: the caller orders it)"""
    if wait:
        import torch
        torch.cuda.current_stream(t.device).synchronize()


def _torch_ptr(t, wait=True):
    """address of a float32 tensor on the library's device, once the work queued on it is done"""
    import torch
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise EuError("a torch tensor handed over as pixels is float32, contiguous and on the device")
    _settle(t, wait)
    return t.data_ptr()


def _stream_handle(stream):
    """a hipStream_t for the C ABI: None (the library's stream), a torch stream or a raw handle"""
    if stream is None:
        return None
    h = getattr(stream, "cuda_stream", stream)
    return C.c_void_p(int(h)) if h else None


_YCBCR_K = {"601": (0.299, 0.114), "709": (0.2126, 0.0722), "2020": (0.2627, 0.0593)}


def ycbcr_matrix(name):
    """(m_rv, m_gu, m_gv, m_bu) of BT.601, BT.709 or BT.2020 as float32 of the float64 values 2(1 - Kr),
    -2 Kb (1 - Kb) / Kg, -2 Kr (1 - Kr) / Kg, 2(1 - Kb) with Kg = 1 - Kr - Kb"""
    if str(name) not in _YCBCR_K:
        raise EuError(f"ycbcr_matrix: {name!r} is none of '601', '709', '2020'")
    kr, kb = _YCBCR_K[str(name)]
    kg = 1.0 - kr - kb
    return tuple(np.float32(v) for v in (2.0 * (1.0 - kr), -2.0 * kb * (1.0 - kb) / kg, -2.0 * kr * (1.0 - kr) / kg,
                                         2.0 * (1.0 - kb)))


def ycbcr_tables(bits, depth=None, full_range=False, msb_aligned=False):
    """(y_table, c_table), 1 << bits float32 each: what a luma / a chroma sample of `depth` significant bits
    (default: bits) becomes. The code c of a stored value v is v, or v >> (bits - depth) when the code sits in the
    high bits (P010). With s = 2**(depth - 8), in float64 and then rounded: limited range (c - 16 s) / (219 s) and
    (c - 128 s) / (224 s); full range c / (2**depth - 1) and (c - 128 s) / (2**depth - 1)."""
    if bits not in (8, 16):
        raise EuError("ycbcr_tables: bits is 8 or 16")
    depth = bits if depth is None else int(depth)
    if depth < 8 or depth > bits:
        raise EuError("ycbcr_tables: depth is 8 .. bits")
    v = np.arange(1 << bits, dtype=np.int64)
    c = (v >> (bits - depth) if msb_aligned else v).astype(np.float64)
    s = 2.0 ** (depth - 8)
    if full_range:
        top = 2.0 ** depth - 1.0
        y, ch = c / top, (c - 128.0 * s) / top
    else:
        y, ch = (c - 16.0 * s) / (219.0 * s), (c - 128.0 * s) / (224.0 * s)
    return y.astype(np.float32), ch.astype(np.float32)


def _plane(a, what, on_device):
    """(address, row pitch in bytes, element stride of a row in samples, bits) of a 2-D plane of samples"""
    if _is_torch(a) != on_device:
        raise EuError("ycbcr: the planes are all numpy arrays or all torch tensors on the device")
    if a.ndim != 2:
        raise EuError(f"ycbcr: {what} is a 2-D plane")
    if on_device:
        import torch
        bits = {torch.uint8: 8, torch.uint16: 16}.get(a.dtype)
        if bits is None or not a.is_cuda:
            raise EuError(f"ycbcr: {what} is uint8 or uint16 and on the device")
        size = bits // 8
        strides = tuple(v * size for v in a.stride())
        addr = a.data_ptr()
    else:
        bits = {np.dtype(np.uint8): 8, np.dtype(np.uint16): 16}.get(a.dtype)
        if bits is None or not a.dtype.isnative:
            raise EuError(f"ycbcr: {what} is uint8 or uint16 in host order")
        size = bits // 8
        strides = tuple(a.strides)
        addr = a.ctypes.data
    h, w = a.shape
    step = strides[1] // size if w > 1 else 1
    if w > 1 and (strides[1] <= 0 or strides[1] % size or step not in (1, 2)):
        raise EuError(f"ycbcr: the samples of a row of {what} are contiguous, or interleaved with one other plane")
    row = ((w - 1) * step + 1) * size
    pitch = strides[0] if h > 1 else row
    if pitch < row:
        raise EuError(f"ycbcr: the rows of {what} overlap or run backwards")
    return addr, pitch, step, bits


def _ycbcr_struct(y, chroma, matrix, y_table, c_table, wait=True):
    """(eu_ycbcr, (h, w), what it points into) for a luma plane, chroma as (cb, cr) or one (ch, cw, 2) array"""
    on_device = _is_torch(y)
    if not on_device:
        y = np.asarray(y)
    if isinstance(chroma, (tuple, list)):
        if len(chroma) != 2:
            raise EuError("ycbcr: chroma is a pair (cb, cr) or one (ch, cw, 2) array")
        cb, cr = chroma if on_device else (np.asarray(chroma[0]), np.asarray(chroma[1]))
    else:
        if not on_device:
            chroma = np.asarray(chroma)
        if chroma.ndim != 3 or chroma.shape[2] != 2:
            raise EuError("ycbcr: chroma is a pair (cb, cr) or one (ch, cw, 2) array")
        cb, cr = chroma[:, :, 0], chroma[:, :, 1]
    ya, yp, ystep, bits = _plane(y, "y", on_device)
    ba, bp, bstep, bbits = _plane(cb, "cb", on_device)
    ra, rp, rstep, rbits = _plane(cr, "cr", on_device)
    if ystep != 1:
        raise EuError("ycbcr: the luma samples of a row are contiguous")
    if bbits != bits or rbits != bits or tuple(cb.shape) != tuple(cr.shape):
        raise EuError("ycbcr: the three planes have one sample type, both chroma planes one shape")
    h, w = y.shape
    ch, cw = cb.shape
    if h > 1 and ch > 1 and bp != rp:
        raise EuError("ycbcr: both chroma planes have one row pitch")
    if cw > 1 and bstep != rstep:
        raise EuError("ycbcr: both chroma planes have one sample step")
    subs = []
    for n, cn, axis in ((w, cw, "width"), (h, ch, "height")):
        if n < 1:
            raise EuError("ycbcr: empty frame")
        if cn == n:
            subs.append(1)
        elif cn == (n + 1) // 2:
            subs.append(2)
        else:
            raise EuError(f"ycbcr: chroma {axis} {cn} fits neither {n} (no subsampling) nor {(n + 1) // 2} (by 2)")
    if y_table is None or c_table is None:
        dy, dc = ycbcr_tables(bits)
        y_table = dy if y_table is None else y_table
        c_table = dc if c_table is None else c_table
    y_table = np.ascontiguousarray(y_table, np.float32)
    c_table = np.ascontiguousarray(c_table, np.float32)
    if y_table.shape != (1 << bits,) or c_table.shape != (1 << bits,):
        raise EuError(f"a table for {bits}-bit samples has {1 << bits} entries")
    if len(matrix) != 4:
        raise EuError("ycbcr: matrix is (m_rv, m_gu, m_gv, m_bu)")
    if on_device:
        _settle(y, wait)
    px = Ycbcr(ya, ba, ra, yp, bp if ch > 1 else max(bp, rp), bstep if cw > 1 else 1, subs[0], subs[1], bits,
               int(on_device), y_table.ctypes.data, c_table.ctypes.data, *[float(np.float32(m)) for m in matrix])
    return px, (h, w), (y, cb, cr, y_table, c_table)


def ycbcr_floats(y, chroma, matrix, y_table, c_table, nchannels=3):
    """eu_hip_ycbcr_floats: the (h, w, nchannels) float32 pixels of a Y'CbCr frame of host planes - what load_ycbcr
    loads, by definition. Host function, no device needed. Arguments as Source.load_ycbcr."""
    px, (h, w), hold = _ycbcr_struct(y, chroma, matrix, y_table, c_table)
    out = np.zeros((h, w, nchannels), np.float32)
    _check(lib().eu_hip_ycbcr_floats(C.byref(px), w, h, nchannels, _ptr(out)))
    return out


def ycbcr_forward(name):
    """(k_r, k_g, k_b, c_u, c_v) of BT.601, BT.709 or BT.2020 as float32 of the float64 values Kr, 1 - Kr - Kb, Kb,
    1 / (2 (1 - Kb)), 1 / (2 (1 - Kr)): the way back from ycbcr_matrix(name)"""
    if str(name) not in _YCBCR_K:
        raise EuError(f"ycbcr_forward: {name!r} is none of '601', '709', '2020'")
    kr, kb = _YCBCR_K[str(name)]
    return tuple(np.float32(v) for v in (kr, 1.0 - kr - kb, kb, 1.0 / (2.0 * (1.0 - kb)), 1.0 / (2.0 * (1.0 - kr))))


def ycbcr_steps(bits, depth=None, full_range=False):
    """(y_steps, c_steps), 1 << bits float32 each: the step tables (eu_ycbcr_out) of the usual quantiser, the inverse
    of ycbcr_tables(bits, depth, full_range). steps[k] is the smallest float32 v whose code
    clip(floor(float64(v) * a + b + 0.5), 0, 2**depth - 1) (NaN: 0) is >= k, found by bisection over the float32 bit
    patterns with that very expression as sample_steps does; steps[0] is -inf, entries behind 2**depth - 1 are NaN.
    With s = 2**(depth - 8): limited range a, b = 219 s, 16 s for luma and 224 s, 128 s for chroma; full range
    2**depth - 1, 0 and 2**depth - 1, 128 s. The codes sit in the LOW bits: a surface with the code in the high bits
    (P010) takes them with shift = bits - depth."""
    if bits not in (8, 16):
        raise EuError("ycbcr_steps: bits is 8 or 16")
    depth = bits if depth is None else int(depth)
    if depth < 8 or depth > bits:
        raise EuError("ycbcr_steps: depth is 8 .. bits")
    n, top = 1 << bits, (1 << depth) - 1
    s = 2.0 ** (depth - 8)
    ab = ((float(top), 0.0), (float(top), 128.0 * s)) if full_range else ((219.0 * s, 16.0 * s), (224.0 * s, 128.0 * s))

    def table(a, b):
        def q(v):
            with np.errstate(invalid="ignore", over="ignore"):
                c = np.floor(v.astype(np.float64) * a + b + 0.5)
                return np.where(np.isnan(c), 0.0, np.clip(c, 0.0, float(top))).astype(np.uint32)

        want = np.arange(1, top + 1, dtype=np.uint32)
        lo = np.full(top, _float_keys(np.float32(-np.inf))[()], np.uint64)
        hi = np.full(top, _float_keys(np.float32(np.inf))[()], np.uint64)
        while (lo < hi).any():
            mid = (lo + hi) // 2
            up = q(_key_floats(mid.astype(np.uint32))) >= want
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid + 1)
        steps = np.full(n, np.nan, np.float32)
        steps[0] = -np.inf
        steps[1:top + 1] = _key_floats(lo.astype(np.uint32))
        return steps

    return table(*ab[0]), table(*ab[1])


def _ycbcr_out_planes(who, out, h, w, subsampling, interleaved, bits, like_torch):
    """(y, chroma) for a frame of h x w pixels: `out` checked against the shapes load_ycbcr takes, or new planes -
    numpy arrays, or torch tensors on the device of `like_torch`"""
    sx, sy = (int(v) for v in subsampling)
    if sx not in (1, 2) or sy not in (1, 2):
        raise EuError(f"{who}: subsampling is (sub_x, sub_y), 1 or 2 each")
    if bits not in (8, 16):
        raise EuError(f"{who}: bits is 8 or 16")
    ch, cw = (h + sy - 1) // sy, (w + sx - 1) // sx
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise EuError(f"{who}: out is (y, chroma)")
        y, chroma = out
    elif like_torch is not None:
        import torch
        dt = {8: torch.uint8, 16: torch.uint16}[bits]
        y = torch.empty((h, w), dtype=dt, device=like_torch.device)
        chroma = (torch.empty((ch, cw, 2), dtype=dt, device=like_torch.device) if interleaved else
                  (torch.empty((ch, cw), dtype=dt, device=like_torch.device),
                   torch.empty((ch, cw), dtype=dt, device=like_torch.device)))
    else:
        dt = _SAMPLE_DTYPE[bits]
        y = np.zeros((h, w), dt)
        chroma = np.zeros((ch, cw, 2), dt) if interleaved else (np.zeros((ch, cw), dt), np.zeros((ch, cw), dt))
    if isinstance(chroma, (tuple, list)):
        if len(chroma) != 2:
            raise EuError(f"{who}: chroma is a pair (cb, cr) or one (ch, cw, 2) array")
        cb, cr = chroma
    else:
        if chroma.ndim != 3 or chroma.shape[2] != 2:
            raise EuError(f"{who}: chroma is a pair (cb, cr) or one (ch, cw, 2) array")
        cb, cr = chroma[:, :, 0], chroma[:, :, 1]
    if tuple(y.shape) != (h, w) or tuple(cb.shape) != (ch, cw) or tuple(cr.shape) != (ch, cw):
        raise EuError(f"{who}: the planes of a {w} x {h} frame are ({h}, {w}) luma and ({ch}, {cw}) chroma samples")
    return y, chroma, cb, cr, sx, sy


def _ycbcr_out_struct(who, forward, y, cb, cr, sx, sy, bits, shift, y_steps, c_steps, wait=True):
    """(eu_ycbcr_out, what it points into) for planes as _ycbcr_out_planes returns them"""
    on_device = _is_torch(y)
    ya, yp, ystep, ybits = _plane(y, "y", on_device)
    ba, bp, bstep, bbits = _plane(cb, "cb", on_device)
    ra, rp, rstep, rbits = _plane(cr, "cr", on_device)
    if ystep != 1:
        raise EuError(f"{who}: the luma samples of a row are contiguous")
    if (ybits, bbits, rbits) != (bits, bits, bits):
        raise EuError(f"{who}: the three planes hold uint{bits} samples")
    ch, cw = cb.shape
    if y.shape[0] > 1 and ch > 1 and bp != rp:
        raise EuError(f"{who}: both chroma planes have one row pitch")
    if cw > 1 and bstep != rstep:
        raise EuError(f"{who}: both chroma planes have one sample step")
    if cw > 1:
        step = bstep
    else:                               # one sample per row: a pair where cb and cr lie side by side in a row
        step = 2 if abs(ra - ba) == bits // 8 and (ch == 1 or min(bp, rp) >= bits // 4) else 1
    if y_steps is None or c_steps is None:
        dy, dc = ycbcr_steps(bits, bits - int(shift) if 0 <= int(shift) <= bits - 8 else None)
        y_steps = dy if y_steps is None else y_steps
        c_steps = dc if c_steps is None else c_steps
    y_steps = np.ascontiguousarray(y_steps, np.float32)
    c_steps = np.ascontiguousarray(c_steps, np.float32)
    if y_steps.shape != (1 << bits,) or c_steps.shape != (1 << bits,):
        raise EuError(f"{who}: a step table for {bits}-bit samples has {1 << bits} entries")
    if len(forward) != 5:
        raise EuError(f"{who}: forward is (k_r, k_g, k_b, c_u, c_v)")
    if on_device:
        _settle(y, wait)
    o = YcbcrOut(ya, ba, ra, yp, bp if ch > 1 else max(bp, rp), step, sx, sy, bits, int(shift), int(on_device),
                 y_steps.ctypes.data, c_steps.ctypes.data, *[float(np.float32(k)) for k in forward])
    return o, (y, cb, cr, y_steps, c_steps)


def _ycbcr_frame(who, frame):
    if not _is_torch(frame) and not (isinstance(frame, np.ndarray) and frame.dtype == np.float32):
        frame = np.ascontiguousarray(frame, np.float32)
    if frame.ndim != 3 or frame.shape[2] not in (3, 4):
        raise EuError(f"{who}: a frame has shape (h, w, 3) or (h, w, 4)")
    return frame


def ycbcr_planes(frame, forward, subsampling=(2, 2), interleaved=False, bits=8, shift=0, y_steps=None, c_steps=None,
                 out=None):
    """eu_hip_ycbcr_planes: the planes of a float frame on the host - what encode_ycbcr makes on the device, by
    definition. Host function, no device needed. Arguments and result as encode_ycbcr, numpy only."""
    frame = _ycbcr_frame("ycbcr_planes", frame)
    if _is_torch(frame):
        raise EuError("ycbcr_planes: a host function, the frame is a numpy array")
    h, w, nch = frame.shape
    y, chroma, cb, cr, sx, sy = _ycbcr_out_planes("ycbcr_planes", out, h, w, subsampling, interleaved, bits, None)
    if h == 0 or w == 0:
        return y, chroma
    o, keep = _ycbcr_out_struct("ycbcr_planes", forward, y, cb, cr, sx, sy, bits, shift, y_steps, c_steps)
    fptr, fstride, f_dev, lead, width, height = _grid(frame, "frame")
    _check(lib().eu_hip_ycbcr_planes(C.c_void_p(fptr), fstride, w, h, nch, C.byref(o)))
    return y, chroma


def encode_ycbcr(frame, forward, subsampling=(2, 2), interleaved=False, bits=8, shift=0, y_steps=None, c_steps=None,
                 out=None, stream=None):
    """eu_hip_encode_ycbcr: a float frame to the planes of a Y'CbCr frame on the device, the mirror of load_ycbcr.
    `frame`: float32 (h, w, 3) or (h, w, 4) (alpha is ignored), a numpy array or a torch tensor on the library's
    device, rows possibly padded. forward: (k_r, k_g, k_b, c_u, c_v), see ycbcr_forward(). subsampling: (sub_x,
    sub_y), 1 or 2 each - the chroma sample is the mean of its pixels, the edge replicated. y_steps / c_steps: float32
    step tables of 1 << bits entries; without them ycbcr_steps(bits, bits - shift) (limited range). The stored sample is
    code << shift (P010: bits 16, shift 6). Returns (y, chroma) in the shapes load_ycbcr takes: chroma is (cb, cr),
    or with `interleaved` one (ch, cw, 2) array (NV12; for NV21 hand over out=(y, (vu[..., 1], vu[..., 0]))). New
    numpy arrays for a numpy frame, new torch tensors for a torch frame, or `out` = (y, chroma), numpy arrays or
    torch tensors on the device with their own strides. With frame and planes on the device the call is asynchronous
    on `stream` (a torch stream or a hipStream_t address; None: the library's stream, after the tensors' current
    stream has been waited for) until sync()."""
    frame = _ycbcr_frame("encode_ycbcr", frame)
    h, w, nch = frame.shape
    y, chroma, cb, cr, sx, sy = _ycbcr_out_planes("encode_ycbcr", out, h, w, subsampling, interleaved, bits,
                                                  frame if _is_torch(frame) else None)
    if h == 0 or w == 0:
        return y, chroma
    o, keep = _ycbcr_out_struct("encode_ycbcr", forward, y, cb, cr, sx, sy, bits, shift, y_steps, c_steps,
                                wait=stream is None)
    if _is_torch(frame) and stream is not None:
        st = tuple(frame.stride())
        if not frame.is_cuda or st[2] != 1 or st[1] != nch or st[0] < w * nch:
            raise EuError("encode_ycbcr: a torch frame is float32 on the device with dense pixels")
        fptr, fstride, f_dev = frame.data_ptr(), st[0] * 4, True
    else:
        fptr, fstride, f_dev, lead, width, height = _grid(frame, "frame")
    _check(lib().eu_hip_encode_ycbcr(C.c_void_p(fptr), fstride, int(f_dev), w, h, nch, C.byref(o), _stream_handle(stream)))
    return y, chroma


def render_ycbcr(args, sources, forward, subsampling=(2, 2), interleaved=False, bits=8, shift=0, y_steps=None,
                 c_steps=None, out=None, stream=None, nchannels=None, row_begin=0, row_end=None, band=None):
    """eu_hip_render_ycbcr: render() of a 3- or 4-channel target with the encode behind it on the device - the planes
    of the rows row_begin .. row_end taken as an image of its own, byte for byte ycbcr_planes(render(...), ...),
    without the float frame leaving the device. Keywords and result as encode_ycbcr; new planes are numpy arrays.
    With `out` on the device the call is asynchronous on `stream` until sync(). Float frames only: no stage output,
    not a tethered job."""
    if not isinstance(sources, (list, tuple)):
        sources = [sources]
    if args.tethered:
        raise EuError("render_ycbcr: a tethered job has its own format (render)")
    t = args.target(nchannels or sources[0].fct.nchannels, row_begin, row_end, 0, band)
    rows, w = t.row_end - t.row_begin, args.out_width
    y, chroma, cb, cr, sx, sy = _ycbcr_out_planes("render_ycbcr", out, rows, w, subsampling, interleaved, bits, None)
    if rows == 0 or w == 0:
        return y, chroma
    o, keep = _ycbcr_out_struct("render_ycbcr", forward, y, cb, cr, sx, sy, bits, shift, y_steps, c_steps,
                                wait=stream is None)
    arr = (C.c_void_p * len(sources))(*[s.handle for s in sources])
    _check(lib().eu_hip_render_ycbcr(C.byref(t), arr, len(sources), C.byref(o), _stream_handle(stream)))
    return y, chroma


def reload_scratch_release():
    """eu_hip_reload_scratch_release: waits for every reload so far and frees the scratch they share"""
    _check(lib().eu_hip_reload_scratch_release())


def facet_alpha_rows(width, height, polygons=(), crop=None, crop_kind=0):
    """eu_hip_facet_alpha_rows: the integer row plan of the alpha plane before the binomial. Returns
    (keep (h, 2), row_start (h + 1), spans (n, 2)): pixel (x, y) is 0 iff x is outside keep[y] or
    inside one of spans[row_start[y]:row_start[y + 1]]. Host function."""
    e, hold = _facet_edit(polygons, crop, crop_kind, 0, False)
    keep = np.zeros((height, 2), np.int32)
    row_start = np.zeros(height + 1, np.int32)
    args = (width, height, e.polygons, e.npolygons, e.crop_kind, e.crop_x0, e.crop_x1, e.crop_y0, e.crop_y1)
    n = _check(lib().eu_hip_facet_alpha_rows(*args, None, None, None, 0))
    spans = np.zeros((n, 2), np.int32)
    _check(lib().eu_hip_facet_alpha_rows(*args, _ptr(keep), _ptr(row_start), _ptr(spans), n))
    return keep, row_start, spans


def facet_alpha_dev(pixels, polygons=(), crop=None, crop_kind=0, shape=None, nchannels=4, want_alpha=True):
    """eu_hip_facet_alpha_dev: facet_alpha on the device. `pixels` ((h, w, 2|4) float32) is edited in
    place: a torch tensor on the library's device where it lies, a numpy array through a device copy.
    pixels=None with shape=(h, w): the alpha plane alone. Returns the plane (numpy) if want_alpha."""
    L = lib()
    tmp = []

    def dev(nbytes):
        q = C.c_void_p()
        _check(L.eu_hip_malloc(C.byref(q), nbytes))
        tmp.append(q)
        return q

    try:
        if pixels is None:
            h, w = shape
            nch, pdev = nchannels, None
        else:
            if pixels.ndim != 3 or (not _is_torch(pixels) and (pixels.dtype != np.float32 or not pixels.flags.c_contiguous)):
                raise EuError("facet_alpha_dev: pixels are (h, w, nchannels) float32, contiguous")
            h, w, nch = pixels.shape
            if _is_torch(pixels):
                pdev = C.c_void_p(_torch_ptr(pixels))
            else:
                pdev = dev(pixels.nbytes)
                _check(L.eu_hip_memcpy_h2d(pdev, _ptr(pixels), pixels.nbytes))
        e, hold = _facet_edit(polygons, crop, crop_kind, nch, True)
        adev = dev(4 * w * h) if want_alpha or pixels is None else None
        _check(L.eu_hip_facet_alpha_dev(pdev, w, h, nch, C.byref(e), adev, None))
        _check(L.eu_hip_sync())
        if pixels is not None and not _is_torch(pixels):
            _check(L.eu_hip_memcpy_d2h(_ptr(pixels), pdev, pixels.nbytes))
        if adev is None:
            return None
        alpha = np.zeros((h, w), np.float32)
        _check(L.eu_hip_memcpy_d2h(_ptr(alpha), adev, alpha.nbytes))
        return alpha
    finally:
        for q in tmp:
            L.eu_hip_free(q)


def cubemap_metrics(face_px, face_fov=math.pi / 2, support_min=8, tile_px=64):
    sec, lf = C.c_int64(), C.c_int64()
    refc, m2p = C.c_double(), C.c_double()
    _check(lib().eu_hip_cubemap_metrics(face_px, face_fov, support_min, tile_px,
                                        C.byref(sec), C.byref(lf), C.byref(refc), C.byref(m2p)))
    return dict(section_px=sec.value, left_frame_px=lf.value, refc_md=refc.value,
                model_to_px=m2p.value)


def container_geometry(degree, bc0, bc1, w, h):
    g = Container()
    _check(lib().eu_hip_container_geometry(degree, bc0, bc1, w, h, C.byref(g)))
    return g


class facet_spec:
    """Host mirror of envutil's facet_spec (envutil_basic.h:432-520): the fields
    the render path reads. Angles in DEGREES here, as on envutil's command
    line; converted to radians when the C struct is built
    (envutil_main.cc:957-960)."""

    def __init__(self, projection, width, height, hfov, nchannels=3, yaw=0.0,
                 pitch=0.0, roll=0.0, brighten=1.0, window=None, lens=None, translation=None, masked=-1):
        self.projection = projection
        self.masked = masked            # --mask_for: -1 ordinary, 0 painted black, 1 painted white
        self.width, self.height = width, height
        self.hfov = hfov
        self.nchannels = nchannels
        self.yaw, self.pitch, self.roll = yaw, pitch, roll
        self.brighten = brighten
        self.window = window or (width, height, 0, 0)
        self.lens = lens or {}          # PTO a, b, c, h, v, g (shear_g), t (shear_t)
        # PTO TrX, TrY, TrZ as x, y, z (model space units), Tpy, Tpp as tp_y, tp_p (+ tp_r), degrees
        self.translation = translation or {}

    def c_struct(self):
        f = Facet()
        f.projection = self.projection
        f.nchannels = self.nchannels
        f.hfov = math.radians(self.hfov)
        f.width, f.height = self.width, self.height
        (f.window_width, f.window_height, f.window_x_offset, f.window_y_offset) = self.window
        f.yaw, f.pitch, f.roll = (math.radians(v) for v in (self.yaw, self.pitch, self.roll))
        f.brighten = self.brighten
        f.step = get_step(self.projection, self.width, self.height, f.hfov)
        for k, v in self.lens.items():
            setattr(f, {"g": "shear_g", "t": "shear_t"}.get(k, k), v)
        f.has_lcp = int(any(self.lens.get(k, 0.0) != 0.0 for k in "abc"))
        f.tr_x, f.tr_y, f.tr_z = (self.translation.get(k, 0.0) for k in ("x", "y", "z"))
        f.tp_y, f.tp_p, f.tp_r = (math.radians(self.translation.get(k, 0.0)) for k in ("tp_y", "tp_p", "tp_r"))
        f.mask_paint = self.masked + 1
        return f


class Source:
    """A source image resident in HBM (the asset_handler entry,
    environment.h:84-227)."""

    def __init__(self, handle, fct, spline_degree=None):
        self.handle = handle
        self.fct = fct
        self.spline_degree = spline_degree

    @staticmethod
    def _float_feed(fct, pixels, masks, crop, crop_kind, wait=True):
        """(address, channels, on_device, eu_facet_edit or None, what they point into) of float pixels"""
        on_device = _is_torch(pixels)
        if not on_device:
            pixels = np.ascontiguousarray(pixels, np.float32)
        # (h, w, channels); (h, w) for the one channel of a facet that gains alpha; else as the facet says
        pch = pixels.shape[2] if pixels.ndim == 3 else 1 if pixels.ndim == 2 and fct.nchannels == 2 else fct.nchannels
        ptr = C.c_void_p(_torch_ptr(pixels, wait)) if on_device else _ptr(pixels)
        if on_device or len(masks) or crop is not None or pch != fct.nchannels:
            e, hold = _facet_edit(masks, crop, crop_kind, pch, on_device)
            return ptr, pch, on_device, e, (pixels, hold)
        return ptr, pch, on_device, None, (pixels,)

    @staticmethod
    def _samples_feed(fct, samples, colour_table, alpha_table, maxval, big_endian, masks, crop, crop_kind, wait=True):
        """(eu_samples, eu_facet_edit or None, what they point into)"""
        on_device = _is_torch(samples)
        if on_device:
            import torch
            bits = {torch.uint8: 8, torch.uint16: 16}.get(samples.dtype)
            if bits is None or not samples.is_cuda or not samples.is_contiguous():
                raise EuError("a torch tensor handed over as samples is uint8 or uint16, contiguous and on the device")
            _settle(samples, wait)
            data = samples.data_ptr()
        else:
            samples = np.asarray(samples)
            bits = {np.dtype(np.uint8): 8, np.dtype(np.uint16): 16}.get(samples.dtype.newbyteorder("="))
            if bits is None:
                raise EuError("samples are uint8 or uint16")
            if bits == 16 and samples.dtype.byteorder == ">":
                samples, big_endian = samples.view(np.uint16), True      # the bytes as they are
            samples = np.ascontiguousarray(samples)
            data = samples.ctypes.data
        n = 1 << bits
        if colour_table is None:
            mv = np.float32(maxval if maxval is not None else n - 1)
            colour_table = np.arange(n, dtype=np.float32) / mv
        tabs = [np.ascontiguousarray(t, np.float32) for t in (colour_table, alpha_table) if t is not None]
        if any(t.shape != (n,) for t in tabs):
            raise EuError(f"a table for {bits}-bit samples has {n} entries")
        # (h, w, channels); (h, w) for the one channel of a facet that gains alpha; else as the facet says
        pch = samples.shape[2] if samples.ndim == 3 else 1 if samples.ndim == 2 and fct.nchannels == 2 else fct.nchannels
        sm = Samples(data, bits, int(bool(big_endian)), pch, int(on_device), tabs[0].ctypes.data,
                     tabs[1].ctypes.data if len(tabs) > 1 else None)
        e, hold = _facet_edit(masks, crop, crop_kind, pch, on_device)
        edited = len(masks) or crop is not None
        return sm, e if edited else None, (samples, tabs, hold)

    @staticmethod
    def _rgbe_feed(quads, colour_table, masks, crop, crop_kind, wait=True):
        """(eu_rgbe, eu_facet_edit or None, what they point into)"""
        on_device = _is_torch(quads)
        if on_device:
            import torch
            if quads.dtype != torch.uint8 or not quads.is_cuda or not quads.is_contiguous():
                raise EuError("a torch tensor handed over as quads is uint8, contiguous and on the device")
            _settle(quads, wait)
            data = quads.data_ptr()
        else:
            quads = np.asarray(quads)
            if quads.dtype != np.uint8:
                raise EuError("quads are uint8")
            quads = np.ascontiguousarray(quads)
            data = quads.ctypes.data
        if quads.ndim < 1 or quads.shape[-1] != 4:
            raise EuError("quads have shape (..., 4): R, G, B, E")
        if colour_table is not None:
            colour_table = np.ascontiguousarray(colour_table, np.float32)
            if colour_table.shape != (65536,):
                raise EuError("a table for RGBE pixels has 65536 entries")
        px = Rgbe(data, int(on_device), colour_table.ctypes.data if colour_table is not None else None)
        e, hold = _facet_edit(masks, crop, crop_kind, 3, on_device)
        edited = len(masks) or crop is not None
        return px, e if edited else None, (quads, colour_table, hold)

    @staticmethod
    def _ycbcr_feed(y, chroma, matrix, y_table, c_table, masks, crop, crop_kind, wait=True):
        """(eu_ycbcr, eu_facet_edit or None, what they point into)"""
        px, shape, hold = _ycbcr_struct(y, chroma, matrix, y_table, c_table, wait)
        e, hold2 = _facet_edit(masks, crop, crop_kind, 3, bool(px.on_device))
        edited = len(masks) or crop is not None
        return px, e if edited else None, (hold, hold2)

    @classmethod
    def _load_pixels(cls, fct, px, e, spline_degree, prefilter_degree, support_min, tile_size, flags):
        """eu_hip_source_load_pixels: the one load for every feed, with flags"""
        if e is not None:
            px.edit = C.cast(C.pointer(e), C.c_void_p)
        cf = fct.c_struct()
        h = C.c_void_p()
        _check(lib().eu_hip_source_load_pixels(C.byref(cf), C.byref(px), spline_degree, prefilter_degree, support_min,
                                               tile_size, flags, C.byref(h)))
        return cls(h, fct, spline_degree)

    @property
    def has_edges(self):
        """the source keeps a distance plane (it was loaded with edges=True)"""
        return bool(self.handle) and bool(lib().eu_hip_source_has_edges(self.handle))

    def edge_device_ptr(self):
        """the device address of the distance plane, or None"""
        p = C.c_void_p()
        _check(lib().eu_hip_source_edge_device_ptr(self.handle, C.byref(p)))
        return p.value

    def edge_distance(self):
        """(h, w) float32: the distance plane of a source loaded with edges=True - per window pixel the distance, in
        source pixels, to the nearest pixel whose alpha is not positive (eu_hip_source_edge_distance)"""
        out = np.zeros((self.fct.window[1], self.fct.window[0]), np.float32)
        _check(lib().eu_hip_source_edge_distance(self.handle, _ptr(out), out.strides[0], 0, None))
        return out

    @classmethod
    def load(cls, fct, pixels, spline_degree, prefilter_degree=None, support_min=8,
             tile_size=64, masks=(), crop=None, crop_kind=0, edges=False):
        """pixels -> braced + prefiltered coefficients, on the device. `pixels`: a numpy array or a
        float32 torch tensor on the library's device. masks (PTO exclude polygons, a list of (xs, ys)),
        crop (x0, x1, y0, y1) with crop_kind 1 rectangular / 2 elliptic: source_t's alpha edit, made on
        the device on the way into the container (eu_hip_source_load_edited); the pixels may then have
        one channel fewer than the facet, which gains its alpha channel here. edges=True (a facet of 2 or 4 channels):
        the source also keeps its distance plane - see edge_distance() -, which the feathered synopses take into the
        blend weight (eu_hip_source_load_pixels with EU_LOAD_EDGES)."""
        if prefilter_degree is None:
            prefilter_degree = spline_degree
        cf = fct.c_struct()
        h = C.c_void_p()
        ptr, pch, on_device, e, hold = cls._float_feed(fct, pixels, masks, crop, crop_kind)
        if edges:
            px = Pixels(PX_FLOATS, ptr, pch, int(on_device), None, None, None, None)
            return cls._load_pixels(fct, px, e, spline_degree, prefilter_degree, support_min, tile_size, LOAD_EDGES)
        if e is not None:
            _check(lib().eu_hip_source_load_edited(C.byref(cf), ptr, C.byref(e), spline_degree, prefilter_degree,
                                                   support_min, tile_size, C.byref(h)))
            return cls(h, fct, spline_degree)
        _check(lib().eu_hip_source_load(C.byref(cf), ptr, spline_degree,
                                        prefilter_degree, support_min, tile_size, C.byref(h)))
        return cls(h, fct, spline_degree)

    @classmethod
    def load_samples(cls, fct, samples, colour_table=None, alpha_table=None, maxval=None, big_endian=False,
                     spline_degree=1, prefilter_degree=None, support_min=8, tile_size=64, masks=(), crop=None,
                     crop_kind=0, edges=False):
        """8- or 16-bit integer samples -> the same source as load() of table[samples], decoded on the device
        (eu_hip_source_load_samples): the samples go up as they are, no float copy is made on the host.
        `samples`: a uint8 / uint16 numpy array or a contiguous torch tensor of those dtypes on the library's
        device, (h, w, channels) or (h, w); big_endian: 16-bit samples are stored high byte first, as in PNM /
        PAM files. colour_table / alpha_table: float32, 256 or 65536 entries - the float each value becomes in
        a colour channel / in the last of 2 or 4 channels (alpha_table None: the colour table). Without tables
        both are v / maxval in float32, maxval defaulting to 255 / 65535. masks, crop, crop_kind as load()."""
        if prefilter_degree is None:
            prefilter_degree = spline_degree
        sm, e, hold = cls._samples_feed(fct, samples, colour_table, alpha_table, maxval, big_endian, masks, crop, crop_kind)
        if edges:
            px = Pixels(PX_SAMPLES, None, 0, 0, C.cast(C.pointer(sm), C.c_void_p), None, None, None)
            return cls._load_pixels(fct, px, e, spline_degree, prefilter_degree, support_min, tile_size, LOAD_EDGES)
        cf = fct.c_struct()
        h = C.c_void_p()
        _check(lib().eu_hip_source_load_samples(C.byref(cf), C.byref(sm), C.byref(e) if e is not None else None,
                                                spline_degree, prefilter_degree, support_min, tile_size, C.byref(h)))
        return cls(h, fct, spline_degree)

    @classmethod
    def load_rgbe(cls, fct, quads, colour_table=None, spline_degree=1, prefilter_degree=None, support_min=8,
                  tile_size=64, masks=(), crop=None, crop_kind=0, edges=False):
        """Radiance RGBE pixels -> the same source as load() of their decoded floats, decoded on the device
        (eu_hip_source_load_rgbe): the quads go up as they are, no float copy is made on the host. `quads`: a uint8
        numpy array or a contiguous torch uint8 tensor on the library's device, (h, w, 4): R, G, B, E. fct.nchannels is
        3, or 4: the facet gains alpha = 1.0 here. colour_table: float32, 65536 entries indexed (E << 8) | mantissa -
        the float a channel becomes; None: mantissa * 2^(E - 136), E == 0 -> 0. masks, crop, crop_kind as load()."""
        if prefilter_degree is None:
            prefilter_degree = spline_degree
        px, e, hold = cls._rgbe_feed(quads, colour_table, masks, crop, crop_kind)
        if edges:
            pp = Pixels(PX_RGBE, None, 0, 0, None, C.cast(C.pointer(px), C.c_void_p), None, None)
            return cls._load_pixels(fct, pp, e, spline_degree, prefilter_degree, support_min, tile_size, LOAD_EDGES)
        cf = fct.c_struct()
        h = C.c_void_p()
        _check(lib().eu_hip_source_load_rgbe(C.byref(cf), C.byref(px), C.byref(e) if e is not None else None,
                                             spline_degree, prefilter_degree, support_min, tile_size, C.byref(h)))
        return cls(h, fct, spline_degree)

    @classmethod
    def load_ycbcr(cls, fct, y, chroma, matrix, y_table=None, c_table=None, spline_degree=1, prefilter_degree=None,
                   support_min=8, tile_size=64, masks=(), crop=None, crop_kind=0, edges=False):
        """The planes of a Y'CbCr frame -> the same source as load() of ycbcr_floats() of them, decoded on the device
        (eu_hip_source_load_ycbcr): the planes go up as their rows lie, no float copy is made on the host. `y`: (h, w)
        uint8 or uint16, a numpy array or a torch tensor on the library's device. `chroma`: a pair (cb, cr) of (ch, cw)
        arrays, or one (ch, cw, 2) array of interleaved Cb, Cr (NV12 / P010; NV21: the pair (a[..., 1], a[..., 0])).
        sub_x and sub_y follow from the shapes: ch, cw equal h, w or their halves rounded up. Row strides are honoured as
        pitches; the samples of a row are contiguous (interleaved chroma: two apart). `matrix`: (m_rv, m_gu, m_gv, m_bu),
        see ycbcr_matrix(). y_table / c_table: float32, 256 or 65536 entries - the float a luma / chroma sample becomes;
        without them ycbcr_tables(bits). Chroma is replicated. fct.nchannels is 3, or 4: the facet gains alpha = 1.0
        here. masks, crop, crop_kind as load()."""
        if prefilter_degree is None:
            prefilter_degree = spline_degree
        px, e, hold = cls._ycbcr_feed(y, chroma, matrix, y_table, c_table, masks, crop, crop_kind)
        if edges:
            pp = Pixels(PX_YCBCR, None, 0, 0, None, None, C.cast(C.pointer(px), C.c_void_p), None)
            return cls._load_pixels(fct, pp, e, spline_degree, prefilter_degree, support_min, tile_size, LOAD_EDGES)
        cf = fct.c_struct()
        h = C.c_void_p()
        _check(lib().eu_hip_source_load_ycbcr(C.byref(cf), C.byref(px), C.byref(e) if e is not None else None,
                                              spline_degree, prefilter_degree, support_min, tile_size, C.byref(h)))
        return cls(h, fct, spline_degree)

    # ---- new pixels into the resident container (eu_hip_source_reload) -----------------------------------------
    def _reload(self, px, e, prefilter_degree, stream):
        if prefilter_degree is None:
            prefilter_degree = self.spline_degree
        if prefilter_degree is None:
            raise EuError("reload: this source does not know its spline degree: give prefilter_degree")
        if e is not None:
            px.edit = C.cast(C.pointer(e), C.c_void_p)
        _check(lib().eu_hip_source_reload(self.handle, C.byref(px), prefilter_degree, _stream_handle(stream)))

    def reload(self, pixels, prefilter_degree=None, masks=(), crop=None, crop_kind=0, stream=None):
        """New float pixels into the resident container, in place (eu_hip_source_reload): afterwards the source is
        what load() makes of `pixels` for this facet - geometry, degree and device address stay. Arguments as load().
        stream: None (the library's stream), a torch stream or a raw hipStream_t; the device work is queued on it, behind
        every render that still reads the container, and later renders go behind it. With a stream a torch tensor's own
        stream is NOT synchronised: the caller orders `stream` behind whatever writes the tensor. Without one the call
        behaves as load(): the tensor's stream is synchronised, the library's used. With device pixels and no masks or
        crop the call does not wait for the device: sync(), or synchronising the stream, says the container is ready."""
        ptr, pch, on_device, e, hold = self._float_feed(self.fct, pixels, masks, crop, crop_kind, wait=stream is None)
        px = Pixels(PX_FLOATS, ptr, pch, int(on_device), None, None, None, None)
        if e is not None and not (len(masks) or crop is not None):
            e = None                      # nothing but the channel count and the side, which px says itself
        self._reload(px, e, prefilter_degree, stream)

    def reload_samples(self, samples, colour_table=None, alpha_table=None, maxval=None, big_endian=False,
                       prefilter_degree=None, masks=(), crop=None, crop_kind=0, stream=None):
        """reload() from 8- or 16-bit integer samples: arguments as load_samples(), stream as reload()."""
        sm, e, hold = self._samples_feed(self.fct, samples, colour_table, alpha_table, maxval, big_endian, masks, crop,
                                         crop_kind, wait=stream is None)
        px = Pixels(PX_SAMPLES, None, 0, 0, C.cast(C.pointer(sm), C.c_void_p), None, None, None)
        self._reload(px, e, prefilter_degree, stream)

    def reload_rgbe(self, quads, colour_table=None, prefilter_degree=None, masks=(), crop=None, crop_kind=0,
                    stream=None):
        """reload() from Radiance RGBE pixels: arguments as load_rgbe(), stream as reload()."""
        rg, e, hold = self._rgbe_feed(quads, colour_table, masks, crop, crop_kind, wait=stream is None)
        px = Pixels(PX_RGBE, None, 0, 0, None, C.cast(C.pointer(rg), C.c_void_p), None, None)
        self._reload(px, e, prefilter_degree, stream)

    def reload_ycbcr(self, y, chroma, matrix, y_table=None, c_table=None, prefilter_degree=None, masks=(), crop=None,
                     crop_kind=0, stream=None):
        """reload() from the planes of a Y'CbCr frame: arguments as load_ycbcr(), stream as reload(). A decoder's
        surface on the device, no masks: nothing waits - the decode, the prefilter and the renders that follow are
        stream-ordered."""
        yc, e, hold = self._ycbcr_feed(y, chroma, matrix, y_table, c_table, masks, crop, crop_kind, wait=stream is None)
        px = Pixels(PX_YCBCR, None, 0, 0, None, None, C.cast(C.pointer(yc), C.c_void_p), None)
        self._reload(px, e, prefilter_degree, stream)

    @classmethod
    def adopt(cls, fct, container, spline_degree, bc0=BC_REFLECT, bc1=BC_REFLECT,
              support_min=8, tile_size=64):
        """upload an already braced + prefiltered container"""
        container = np.ascontiguousarray(container, np.float32)
        cf = fct.c_struct()
        h = C.c_void_p()
        _check(lib().eu_hip_source_adopt(C.byref(cf), _ptr(container), spline_degree, bc0,
                                         bc1, support_min, tile_size, C.byref(h)))
        return cls(h, fct, spline_degree)

    @classmethod
    def alloc(cls, fct, spline_degree, support_min=8, tile_size=64):
        """an unfilled container in HBM (to be filled by a broadcast)"""
        cf = fct.c_struct()
        h = C.c_void_p()
        _check(lib().eu_hip_source_alloc(C.byref(cf), spline_degree, support_min, tile_size,
                                         C.byref(h)))
        return cls(h, fct, spline_degree)

    def update_facet(self, fct):
        """the facet's geometry changed (orientation, hfov, lens, brighten): rebuild the
        evaluator / mount parameters, keep the resident coefficients"""
        _check(lib().eu_hip_source_update_facet(self.handle, C.byref(fct.c_struct())))
        self.fct = fct

    def device_ptr(self):
        p = C.c_void_p()
        n = C.c_size_t()
        _check(lib().eu_hip_source_device_ptr(self.handle, C.byref(p), C.byref(n)))
        return p.value, n.value

    def info(self):
        g = Container()
        n = C.c_int()
        _check(lib().eu_hip_source_info(self.handle, C.byref(g), C.byref(n)))
        return g, n.value

    def download(self):
        g, n = self.info()
        out = np.zeros((g.shape[1], g.shape[0], n), np.float32)
        _check(lib().eu_hip_source_download(self.handle, _ptr(out), out.size))
        return out

    def release(self):
        if self.handle:
            lib().eu_hip_source_release(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class arguments:
    """Host mirror of the target half of envutil's global `args`
    (envutil_basic.h:633-705): projection, size, hfov -> extent, camera
    orientation (degrees), spline degree, twining."""

    def __init__(self, projection, width, height, hfov, yaw=0.0, pitch=0.0, roll=0.0,
                 spline_degree=1, prefilter_degree=None, twine=0, twine_width=1.0,
                 twine_sigma=0.0, twine_threshold=0.0, support_min=8, tile_size=64,
                 crop=None, tethered=False, synopsis="panorama", single=None, feather=0.0, bands=0):
        # store_cropped + p_crop_x0/x1/y0/y1 (envutil_basic.h:684-687) as
        # (x0, x1, y0, y1); tethered: the job writes packed sRGBA8 words
        # (args.p_screen_data, envutil_payload.cc:524-530)
        self.store_cropped = crop is not None
        self.p_crop = tuple(crop) if crop is not None else None
        self.tethered = tethered
        # args.synopsis (envutil_main.cc:232): how several facets are composed, "panorama" or "hdr_merge" - and
        # "feather", this project's own: feathered seams (eu_hip.h, eu_target::feather)
        # and "multiband", also this project's own: Burt-Adelson blending over `bands` pyramid levels (eu_target::bands)
        if synopsis not in ("panorama", "hdr_merge", "feather", "multiband"):
            raise ValueError("synopsis must be panorama, hdr_merge, feather or multiband")
        self.synopsis = synopsis
        # the pyramid levels of the multiband synopsis above level 0; 0: as many as the frame allows, 8 at the most
        if int(bands) != bands or bands < 0:
            raise ValueError("bands must be a whole number of pyramid levels, 0 for the default")
        self.bands = int(bands)
        # the width of the feathering ramp in source pixels; 0: half the shorter side of each facet's window
        feather = float(feather)
        if not math.isfinite(feather) or feather < 0.0:
            raise ValueError("feather must be a finite width in source pixels, 0 for the default")
        self.feather = feather
        # args.single: the facet_spec this target recreates ((facet_base&) args = fspec, envutil_main.cc:1161-1180);
        # projection, size, hfov and orientation of the target must be the facet's own (see for_single)
        self.single = single
        self.projection = projection
        self.width, self.height = width, height
        self.hfov = hfov
        self.yaw, self.pitch, self.roll = yaw, pitch, roll
        self.spline_degree = spline_degree
        self.prefilter_degree = spline_degree if prefilter_degree is None else prefilter_degree
        self.twine = twine
        self.twine_width, self.twine_sigma = twine_width, twine_sigma
        self.twine_threshold = twine_threshold
        self.support_min, self.tile_size = support_min, tile_size
        # envutil_main.cc:1203-1232
        self.extent = get_extent(projection, width, height, math.radians(hfov))
        self.step = (self.extent[1] - self.extent[0]) / width
        self.twine_spread = None
        if twine:
            # arguments::twine_setup, envutil_main.cc:1405-1616 (explicit twine)
            self.twine_spread = make_spread(twine, twine, twine_width, twine_sigma,
                                            twine_threshold)

    @classmethod
    def for_single(cls, fct, **kw):
        """the target of a --single job: the facet's own geometry taken over as target geometry"""
        return cls(fct.projection, fct.width, fct.height, fct.hfov, yaw=fct.yaw, pitch=fct.pitch, roll=fct.roll,
                   single=fct, **kw)

    def target(self, nchannels, row_begin=0, row_end=None, stage=0, band=None):
        """band = (band_rows, band_count, band_index): this call renders the
        interleaved row bands of one part (eu_target.band_*); rows are local"""
        t = Target()
        t.projection = self.projection
        t.width, t.height = self.width, self.height
        t.x0, t.x1, t.y0, t.y1 = (float(v) for v in self.extent)
        t.yaw, t.pitch, t.roll = (math.radians(v) for v in (self.yaw, self.pitch, self.roll))
        t.nchannels = nchannels
        if self.twine_spread is not None:
            t.ntaps = len(self.twine_spread)
            t.taps = self.twine_spread.ctypes.data_as(C.POINTER(C.c_float))
        if self.store_cropped:
            x0, x1, y0, y1 = self.p_crop
            t.crop_x0, t.crop_y0, t.crop_w, t.crop_h = x0, y0, x1 - x0, y1 - y0
        t.out_format = OUT_SRGBA8 if self.tethered else OUT_FLOAT
        t.synopsis = {"panorama": SYN_PANORAMA, "hdr_merge": SYN_HDR_MERGE, "feather": SYN_FEATHER,
                      "multiband": SYN_MULTIBAND}[self.synopsis]
        t.feather = self.feather
        t.bands = self.bands
        if self.single is not None:
            self._single_c = self.single.c_struct()          # kept alive with the arguments object
            t.single = C.pointer(self._single_c)
        nrows = self.out_height
        if band is not None and band[1] > 1:
            t.band_rows, t.band_count, t.band_index = band
            nrows = band_rows(self.out_height, *band)
        t.row_begin = row_begin
        t.row_end = nrows if row_end is None else row_end
        t.stage = stage
        return t

    @property
    def out_width(self):
        return self.p_crop[1] - self.p_crop[0] if self.store_cropped else self.width

    @property
    def out_height(self):
        return self.p_crop[3] - self.p_crop[2] if self.store_cropped else self.height


def layout_segments(args, sources, nchannels=None):
    """(seg_rows, flags): flags[k] = 1 where rows [k * seg_rows, (k + 1) * seg_rows) of the
    job's frame are rendered with the tile layout and cost about 1.55-2x the others
    (eu_hip_layout_segments); flags is empty when the job has no such structure"""
    if not isinstance(sources, (list, tuple)):
        sources = [sources]
    if len(sources) != 1:
        return 512, np.zeros(0, np.uint8)
    nch = nchannels or sources[0].fct.nchannels
    t = args.target(nch)
    arr = (C.c_void_p * 1)(sources[0].handle)
    flags = np.zeros(65536, np.uint8)
    seg = C.c_int(0)
    n = lib().eu_hip_layout_segments(C.byref(t), arr, 1, flags.ctypes.data_as(C.c_void_p), flags.size,
                                     C.byref(seg))
    _check(n if n < 0 else 0)
    return seg.value, flags[:n].copy()


def band_rows(height, rows, count, index):
    """local rows of part `index` when `height` rows are dealt out in bands of
    `rows` rows to `count` parts (eu_hip_band_rows)"""
    return lib().eu_hip_band_rows(height, rows, count, index)


def band_frame_rows(height, rows, count, index):
    """frame row of every local row of that part, in order (numpy int64)"""
    y = np.arange(height)
    return y[(y // rows) % count == index] if count > 1 else y


def render(args, sources, nchannels=None, row_begin=0, row_end=None, stage=0, out=None, band=None):
    """zimt::process(shape, get, act, put, bill) for rows [row_begin, row_end):
    returns (rows, width, nch) float32 on the host - (rows, width) uint32
    sRGBA8 words for a tethered job; width/rows are those of the crop window
    when args.store_cropped."""
    if not isinstance(sources, (list, tuple)):
        sources = [sources]
    nch = nchannels or sources[0].fct.nchannels
    t = args.target(nch, row_begin, row_end, stage, band)
    rows = t.row_end - t.row_begin
    w = args.out_width
    # stage 1: rays, 2: source coordinates, 3 / 4: the x- / y-biased neighbour rays of a twined job
    if args.tethered:
        och = 1
        if out is None:
            out = np.zeros((rows, w), np.uint32)
    else:
        och = 3 if stage else nch
        if out is None:
            out = np.zeros((rows, w, och), np.float32)
    arr = (C.c_void_p * len(sources))(*[s.handle for s in sources])
    _check(lib().eu_hip_render(C.byref(t), arr, len(sources), out.ctypes.data_as(C.c_void_p),
                               w * och * 4, 0, None))
    return out


def multiband_levels(width, height, bands=0, wrap=False):
    """eu_hip_multiband_levels: the pyramid levels above level 0 that a width x height frame gets for `bands`"""
    return _check(lib().eu_hip_multiband_levels(width, height, bands, int(bool(wrap))))


def multiband_scratch_bytes(args, nsources, nchannels=3):
    """eu_hip_multiband_scratch_bytes: device scratch of a multiband job of `nsources` facets on this target"""
    t = args.target(nchannels)
    return int(lib().eu_hip_multiband_scratch_bytes(C.byref(t), nsources))


def multiband_scratch_release():
    """eu_hip_multiband_scratch_release: waits for every multiband job so far and frees the scratch they share"""
    _check(lib().eu_hip_multiband_scratch_release())


def _strided(a, what, tail):
    """(address, strides in bytes, on_device) of a float32 array, numpy or torch on the device, whose last
    len(tail) axes are dense with the shape `tail`"""
    dev = _is_torch(a)
    if dev:
        import torch
        if not a.is_cuda or a.dtype != torch.float32:
            raise EuError(f"blend_layers: {what} is float32, numpy or on the device")
        strides = tuple(4 * k for k in a.stride())
        _settle(a)
        ptr = a.data_ptr()
    else:
        if a.dtype != np.float32:
            raise EuError(f"blend_layers: {what} is float32")
        strides, ptr = tuple(a.strides), a.ctypes.data
    dense = 4
    for n, st in zip((1,) + tuple(tail[:0:-1]), strides[::-1]):
        dense *= n
        if st != dense:
            raise EuError(f"blend_layers: the pixels of {what} are dense, only rows and pictures may be padded")
    return ptr, strides, dev


def blend_layers(colour, weight, bands=0, wrap=False, out=None, stream=None):
    """eu_hip_blend_layers: multi-band blending of the caller's own remapped pictures - the pyramid a multiband render
    runs behind its stage A (eu_hip.h, eu_target::bands). colour (N, H, W, C) plays the facets' colour, weight
    (N, H, W) their weight Q (what is not positive counts as 0); float32, both numpy or both torch tensors on the
    library's device; rows and pictures may be padded. wrap: column indices wrap (a 360-degree frame). Returns the
    (H, W, C) frame: a new numpy array (a new device tensor for device input), or `out`, numpy or torch, rows may be
    padded. With everything on the device the call is asynchronous on `stream` until sync()."""
    if not _is_torch(colour):
        colour, weight = np.asarray(colour), np.asarray(weight)
    if _is_torch(colour) != _is_torch(weight):
        raise EuError("blend_layers: colour and weight lie on the same side")
    if colour.ndim != 4 or weight.ndim != 3 or tuple(colour.shape[:3]) != tuple(weight.shape):
        raise EuError("blend_layers: colour is (N, H, W, C) and weight (N, H, W)")
    n, h, w, c = (int(k) for k in colour.shape)
    cptr, cst, dev = _strided(colour, "colour", (w, c))
    wptr, wst, _ = _strided(weight, "weight", (w,))
    if out is None:
        if dev:
            import torch
            out = torch.empty((h, w, c), dtype=torch.float32, device=colour.device)
        else:
            out = np.zeros((h, w, c), np.float32)
    if tuple(out.shape) != (h, w, c):
        raise EuError(f"blend_layers: out has shape {tuple(out.shape)}, expected {(h, w, c)}")
    optr, ost, o_dev = _strided(out, "out", (w, c))
    _check(lib().eu_hip_blend_layers(C.c_void_p(cptr), cst[1], cst[0], C.c_void_p(wptr), wst[1], wst[0], int(dev), n, w, h, c,
                                     int(bands), int(bool(wrap)), C.c_void_p(optr), ost[0], int(o_dev), _stream_handle(stream)))
    return out


class Encode(C.Structure):
    """struct eu_encode"""
    _fields_ = [("bits", C.c_int32), ("big_endian", C.c_int32),
                ("colour_steps", C.c_void_p), ("alpha_steps", C.c_void_p)]


def _float_keys(v):
    """float32 -> uint32 keys in the order of the floats' values (-inf lowest, +inf highest of the numbers)"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _key_floats(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def sample_steps(bits=8, maxval=None):
    """The step table (eu_encode) of the linear default: steps[k] is the smallest float32 v whose code
    Q(v) = trunc(clip(v, 0, 1) * maxval + 0.5), evaluated in float32 (NaN: 0), is >= k - found by bisection over
    the float32 bit patterns from -inf to +inf, with that very expression; steps[0] is -inf, entries above maxval
    are NaN. 1 << bits float32 values; maxval defaults to 255 / 65535."""
    if bits not in (8, 16):
        raise EuError("sample_steps: bits is 8 or 16")
    n = 1 << bits
    maxval = n - 1 if maxval is None else int(maxval)
    if not 1 <= maxval < n:
        raise EuError(f"sample_steps: maxval is 1 .. {n - 1}")
    mv, half = np.float32(maxval), np.float32(0.5)

    def q(v):
        with np.errstate(invalid="ignore"):
            c = np.minimum(np.maximum(v, np.float32(0)), np.float32(1))
            return (c * mv + half).astype(np.uint32)

    want = np.arange(1, maxval + 1, dtype=np.uint32)
    lo = np.full(maxval, _float_keys(np.float32(-np.inf))[()], np.uint64)
    hi = np.full(maxval, _float_keys(np.float32(np.inf))[()], np.uint64)
    while (lo < hi).any():
        mid = (lo + hi) // 2
        up = q(_key_floats(mid.astype(np.uint32))) >= want
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid + 1)
    steps = np.full(n, np.nan, np.float32)
    steps[0] = -np.inf
    steps[1:maxval + 1] = _key_floats(lo.astype(np.uint32))
    return steps


_SAMPLE_DTYPE = {8: np.uint8, 16: np.uint16}


def _encode_struct(who, bits, colour_steps, alpha_steps, maxval, big_endian):
    """(eu_encode, arrays it points into); without tables the linear default of sample_steps(bits, maxval)"""
    if bits not in (8, 16):
        raise EuError(f"{who}: bits is 8 or 16")
    n = 1 << bits
    if colour_steps is None:
        colour_steps = sample_steps(bits, maxval)
    elif maxval is not None:
        raise EuError(f"{who}: maxval belongs to the default table; a table of the caller's says its own")
    tabs = [np.ascontiguousarray(t, np.float32) for t in (colour_steps, alpha_steps) if t is not None]
    if any(t.shape != (n,) for t in tabs):
        raise EuError(f"{who}: a step table for {bits}-bit samples has {n} entries")
    e = Encode(bits, int(bool(big_endian)), tabs[0].ctypes.data, tabs[1].ctypes.data if len(tabs) > 1 else None)
    return e, tabs


def _sample_rows(who, a, shape, bits):
    """`a`, (rows, width, channels) samples of `bits` bits, numpy or torch on the device, dense pixels, rows possibly
    padded: (address, row stride in bytes, on_device)"""
    if tuple(a.shape) != tuple(shape):
        raise EuError(f"{who}: out has shape {tuple(a.shape)}, expected {tuple(shape)}")
    size = bits // 8
    if _is_torch(a):
        import torch
        if not a.is_cuda or a.dtype != {8: torch.uint8, 16: torch.uint16}[bits]:
            raise EuError(f"{who}: out is uint{bits} and on the device")
        st = tuple(v * size for v in a.stride())
        on_device, ptr = True, a.data_ptr()
    else:
        if not isinstance(a, np.ndarray) or a.dtype.newbyteorder("=") != np.dtype(_SAMPLE_DTYPE[bits]):
            raise EuError(f"{who}: out is a uint{bits} array")
        st, on_device, ptr = tuple(a.strides), False, a.ctypes.data
    rows, w, c = shape
    if rows and w and c and (st[2] != size or st[1] != size * c or (rows > 1 and st[0] < w * c * size)):
        raise EuError(f"{who}: out has dense pixels; only its rows may be padded")
    if on_device:
        import torch
        torch.cuda.current_stream(a.device).synchronize()
    return ptr, (st[0] if rows > 1 else w * c * size), on_device


def encode_samples(frame, colour_steps=None, alpha_steps=None, bits=8, maxval=None, big_endian=False, out=None,
                   stream=None):
    """eu_hip_encode_samples: float pixels to 8- or 16-bit samples on the device. `frame`: float32, shape
    (..., channels) with 1..4 channels, a numpy array or a torch tensor on the library's device (_grid's layouts:
    contiguous, or three axes with padded rows) - the result of render(), render_rays() or render_views().
    colour_steps / alpha_steps: float32 step tables of 1 << bits entries (eu_hip.h: eu_encode; alpha_steps is for
    the last of 2 or 4 channels, None: the colour table); without tables the linear default sample_steps(bits,
    maxval), which equals (clip(v, 0, 1) * maxval + 0.5).astype(...) evaluated in float32. big_endian: 16-bit
    samples are written high byte first, as PNM / PAM files hold them. Returns samples of the frame's shape: a new
    numpy array for a numpy frame, a new torch tensor on the device for a torch frame, or `out` (numpy or torch,
    rows may be padded). With frame and out on the device the call is asynchronous on `stream` (a hipStream_t
    address; None: the library's stream) until sync()."""
    if not _is_torch(frame) and not (isinstance(frame, np.ndarray) and frame.dtype == np.float32):
        frame = np.ascontiguousarray(frame, np.float32)
    if frame.ndim < 1 or not 1 <= frame.shape[-1] <= 4:
        raise EuError("encode_samples: a frame has shape (..., channels), 1 to 4 channels")
    e, keep = _encode_struct("encode_samples", bits, colour_steps, alpha_steps, maxval, big_endian)
    fptr, fstride, f_dev, lead, width, height = _grid(frame, "frame")
    nch = frame.shape[-1]
    if out is None:
        if f_dev:
            import torch
            out = torch.empty(tuple(frame.shape), dtype={8: torch.uint8, 16: torch.uint16}[bits], device=frame.device)
        else:
            out = np.zeros(frame.shape, _SAMPLE_DTYPE[bits])
    if tuple(out.shape) != tuple(frame.shape):
        raise EuError(f"encode_samples: out has shape {tuple(out.shape)}, expected {tuple(frame.shape)}")
    flat = out if out.ndim == 3 and tuple(out.shape[:2]) == (height, width) else out.reshape(height, width, nch)
    optr, ostride, o_dev = _sample_rows("encode_samples", flat, (height, width, nch), bits)
    _check(lib().eu_hip_encode_samples(C.c_void_p(fptr), fstride, int(f_dev), width, height, nch, C.byref(e),
                                       C.c_void_p(optr), ostride, int(o_dev), C.c_void_p(stream) if stream else None))
    return out


def render_samples(args, sources, nchannels=None, row_begin=0, row_end=None, colour_steps=None, alpha_steps=None,
                   bits=8, maxval=None, big_endian=False, out=None, band=None, stream=None):
    """eu_hip_render_samples: render() with the encode behind it on the device - (rows, width, nch) uint8 / uint16,
    byte for byte encode_samples(render(...), ...) with the same tables, without the float frame leaving the device.
    Tables, bits, maxval and big_endian as encode_samples. Returns a new numpy array, or `out` (numpy, or a torch
    tensor of that dtype on the library's device; rows may be padded); with `out` on the device the call is
    asynchronous on `stream` until sync(). Float frames only: no stage output, not a tethered job."""
    if not isinstance(sources, (list, tuple)):
        sources = [sources]
    if args.tethered:
        raise EuError("render_samples: a tethered job has its own format (render)")
    nch = nchannels or sources[0].fct.nchannels
    t = args.target(nch, row_begin, row_end, 0, band)
    rows, w = t.row_end - t.row_begin, args.out_width
    e, keep = _encode_struct("render_samples", bits, colour_steps, alpha_steps, maxval, big_endian)
    if out is None:
        out = np.zeros((rows, w, nch), _SAMPLE_DTYPE[bits])
    optr, ostride, o_dev = _sample_rows("render_samples", out, (rows, w, nch), bits)
    arr = (C.c_void_p * len(sources))(*[s.handle for s in sources])
    _check(lib().eu_hip_render_samples(C.byref(t), arr, len(sources), C.byref(e), C.c_void_p(optr), ostride, int(o_dev),
                                       C.c_void_p(stream) if stream else None))
    return out


def encode_rgbe(frame, out=None, stream=None):
    """eu_hip_encode_rgbe: float pixels to Radiance RGBE quads on the device. `frame`: float32, shape (..., 3), a numpy
    array or a torch tensor on the library's device (_grid's layouts) - the result of render(), render_rays() or
    render_views(). Returns uint8 quads of shape (..., 4) - R, G, B, E -: a new numpy array for a numpy frame, a new
    torch tensor on the device for a torch frame, or `out` (numpy or torch, rows may be padded, a 4-byte boundary).
    With frame and out on the device the call is asynchronous on `stream` (a hipStream_t address; None: the
    library's stream) until sync()."""
    if not _is_torch(frame) and not (isinstance(frame, np.ndarray) and frame.dtype == np.float32):
        frame = np.ascontiguousarray(frame, np.float32)
    if frame.ndim < 1 or frame.shape[-1] != 3:
        raise EuError("encode_rgbe: a frame has shape (..., 3)")
    fptr, fstride, f_dev, lead, width, height = _grid(frame, "frame")
    shape = tuple(frame.shape[:-1]) + (4,)
    if out is None:
        if f_dev:
            import torch
            out = torch.empty(shape, dtype=torch.uint8, device=frame.device)
        else:
            out = np.zeros(shape, np.uint8)
    if tuple(out.shape) != shape:
        raise EuError(f"encode_rgbe: out has shape {tuple(out.shape)}, expected {shape}")
    flat = out if out.ndim == 3 and tuple(out.shape[:2]) == (height, width) else out.reshape(height, width, 4)
    optr, ostride, o_dev = _sample_rows("encode_rgbe", flat, (height, width, 4), 8)
    _check(lib().eu_hip_encode_rgbe(C.c_void_p(fptr), fstride, int(f_dev), width, height, C.c_void_p(optr), ostride,
                                    int(o_dev), C.c_void_p(stream) if stream else None))
    return out


def render_rgbe(args, sources, nchannels=None, row_begin=0, row_end=None, out=None, band=None, stream=None):
    """eu_hip_render_rgbe: render() of a 3-channel target with the encode behind it on the device - (rows, width, 4)
    uint8 quads, byte for byte encode_rgbe(render(...)), without the float frame leaving the device. Returns a new
    numpy array, or `out` (numpy, or a torch uint8 tensor on the library's device; rows may be padded); with `out` on
    the device the call is asynchronous on `stream` until sync(). Float frames only: no stage output, not a tethered
    job."""
    if not isinstance(sources, (list, tuple)):
        sources = [sources]
    if args.tethered:
        raise EuError("render_rgbe: a tethered job has its own format (render)")
    t = args.target(nchannels or sources[0].fct.nchannels, row_begin, row_end, 0, band)    # the library asks for 3
    rows, w = t.row_end - t.row_begin, args.out_width
    if out is None:
        out = np.zeros((rows, w, 4), np.uint8)
    optr, ostride, o_dev = _sample_rows("render_rgbe", out, (rows, w, 4), 8)
    arr = (C.c_void_p * len(sources))(*[s.handle for s in sources])
    _check(lib().eu_hip_render_rgbe(C.byref(t), arr, len(sources), C.c_void_p(optr), ostride, int(o_dev),
                                    C.c_void_p(stream) if stream else None))
    return out


def _grid(a, what):
    """a float32 array of shape (..., k), numpy or torch on the device, as a height x width grid of k floats:
    (address, row stride in bytes, on_device, leading shape, width, height). The leading axes are folded into
    rows of the last of them (one axis: a flat list, height 1). A three-axis array whose rows are padded -
    a[:, :w, :] of a wider array - is used in place with its row stride; everything else must be contiguous."""
    on_device = _is_torch(a)
    lead = tuple(a.shape[:-1])
    k = a.shape[-1]
    n = 1
    for d in lead:
        n *= d
    width = lead[-1] if len(lead) >= 2 else n
    height = n // width if width else 0
    stride = width * k * 4
    if on_device:
        st = tuple(a.stride())
        padded = a.ndim == 3 and st[2] == 1 and st[1] == k and st[0] >= width * k
        if padded:
            import torch
            if not a.is_cuda or a.dtype != torch.float32:
                raise EuError(f"render_rays: {what} is float32 and on the device")
            torch.cuda.current_stream(a.device).synchronize()
            return a.data_ptr(), st[0] * 4, True, lead, width, height
        return _torch_ptr(a), stride, True, lead, width, height
    if a.dtype != np.float32:
        raise EuError(f"render_rays: {what} is float32")
    if a.ndim == 3 and a.strides[2] == 4 and a.strides[1] == 4 * k and a.strides[0] >= stride and a.strides[0] % 4 == 0:
        return a.ctypes.data, a.strides[0], False, lead, width, height
    if not a.flags.c_contiguous:
        raise EuError(f"render_rays: {what} is contiguous, or a three-axis array with padded rows")
    return a.ctypes.data, stride, False, lead, width, height


def _rays_struct(source, rays, nchannels, taps):
    """(eu_rays, leading shape, objects it points into) for rays (..., 3) or ninepacks (..., 9)"""
    if not _is_torch(rays) and not (isinstance(rays, np.ndarray) and rays.dtype == np.float32):
        rays = np.ascontiguousarray(rays, np.float32)
    if rays.ndim < 1 or rays.shape[-1] not in (3, 9):
        raise EuError("render_rays: rays have shape (..., 3), ninepacks (..., 9)")
    ptr, stride, on_device, lead, width, height = _grid(rays, "rays")
    r = Rays()
    r.width, r.height, r.ninputs = width, height, rays.shape[-1]
    r.nchannels = nchannels or source.fct.nchannels
    keep = [rays]
    if taps is not None:
        taps = np.ascontiguousarray(taps, np.float32).reshape(-1, 3)
        keep.append(taps)
        r.ntaps, r.taps = len(taps), taps.ctypes.data_as(C.POINTER(C.c_float))
    r.rays, r.ray_row_stride_bytes, r.rays_on_device = ptr, stride, int(on_device)
    return r, lead, keep


def render_rays(source, rays, nchannels=None, taps=None, out=None, stream=None):
    """eu_hip_render_rays: `act` alone - the resident source evaluated at the caller's rays, three floats
    x, y, z in the SOURCE's frame (what render(..., stage=1) returns; no facet or camera orientation is
    applied), or at ninepacks {ray, x-neighbour, y-neighbour} with `taps` = make_spread(...). `rays`: numpy
    or a float32 torch tensor on the library's device, shape (..., 3) or (..., 9). Returns the rays' leading
    shape plus a channel axis: a new numpy array, or `out` (numpy or torch). With rays and `out` both on the
    device the call is asynchronous on `stream` (a hipStream_t address; None: the library's stream) until
    sync(). A ray with a non-finite component, or with all three zero, is a miss: zeros."""
    r, lead, keep = _rays_struct(source, rays, nchannels, taps)
    shape = lead + (r.nchannels,)
    if out is None:
        out = np.zeros(shape, np.float32)
    if tuple(out.shape) != shape:
        raise EuError(f"render_rays: out has shape {tuple(out.shape)}, expected {shape}")
    optr, ostride, out_dev, _, _, _ = _grid(out, "out")
    _check(lib().eu_hip_render_rays(C.byref(r), source.handle, C.c_void_p(optr), ostride, int(out_dev),
                                    C.c_void_p(stream) if stream else None))
    return out


def render_rays_timed(source, rays, out_dev_ptr, iters, nchannels=None, taps=None):
    """kernel-only timing of render_rays with HIP events on the library's stream. `rays`: a torch tensor on
    the device, or numpy (copied to the device for the call); the output stays in HBM at out_dev_ptr, dense.
    Returns mean milliseconds per launch."""
    L = lib()
    tmp = C.c_void_p()
    try:
        r, lead, keep = _rays_struct(source, rays, nchannels, taps)
        if not r.rays_on_device:
            host = np.ascontiguousarray(keep[0])
            _check(L.eu_hip_malloc(C.byref(tmp), host.nbytes))
            _check(L.eu_hip_memcpy_h2d(tmp, _ptr(host), host.nbytes))
            r.rays, r.rays_on_device, r.ray_row_stride_bytes = tmp.value, 1, r.width * r.ninputs * 4
        ms = C.c_float()
        _check(L.eu_hip_render_rays_timed(C.byref(r), source.handle, C.c_void_p(out_dev_ptr),
                                          r.width * r.nchannels * 4, iters, C.byref(ms)))
        return ms.value
    finally:
        if tmp:
            L.eu_hip_free(tmp)


def _views_struct(args, views):
    """eu_view[] for (yaw, pitch, roll) or (yaw, pitch, roll, hfov) in degrees; args.hfov where a view gives none"""
    arr = (View * max(len(views), 1))()
    for k, v in enumerate(views):
        v = tuple(v)
        if len(v) not in (3, 4):
            raise EuError("render_views: a view is (yaw, pitch, roll) or (yaw, pitch, roll, hfov), degrees")
        hfov = v[3] if len(v) == 4 else args.hfov
        e = args.extent if hfov == args.hfov else get_extent(args.projection, args.width, args.height, math.radians(hfov))
        arr[k].yaw, arr[k].pitch, arr[k].roll = (math.radians(float(a)) for a in v[:3])
        arr[k].x0, arr[k].x1, arr[k].y0, arr[k].y1 = (float(a) for a in e)
    return arr


def _views_args(args, who):
    if args.store_cropped or args.tethered or args.single is not None:
        raise EuError(f"{who}: whole float frames of an ordinary target (no crop, not tethered, no single)")


def _frames(a, what):
    """a float32 (N, H, W, C) array, numpy or torch on the device, whose last two axes are dense: (address, row
    stride, view stride in bytes, on_device). Padded rows and padded views are used in place."""
    on_device = _is_torch(a)
    n, h, w, c = a.shape
    if on_device:
        import torch
        if not a.is_cuda or a.dtype != torch.float32:
            raise EuError(f"render_views: {what} is float32 and on the device")
        st = tuple(4 * v for v in a.stride())
    else:
        if a.dtype != np.float32:
            raise EuError(f"render_views: {what} is float32")
        st = tuple(a.strides)
    if a.size == 0:                 # nothing to stride over
        st = (h * w * c * 4, w * c * 4, c * 4, 4)
    row = st[1] if h > 1 else max(st[1], w * c * 4)
    view = st[0] if n > 1 else max(st[0], h * row)
    if n and h and w and (st[3] != 4 or st[2] != 4 * c or row < w * c * 4 or row % 4 or view < h * row or view % 4):
        raise EuError(f"render_views: {what} has dense pixels; only its rows and views may be padded")
    if on_device:
        import torch
        torch.cuda.current_stream(a.device).synchronize()
        return a.data_ptr(), row, view, True
    return a.ctypes.data, row, view, False


def render_views(args, views, source, nchannels=None, out=None, stream=None):
    """eu_hip_render_views / eu_hip_render_views_multi: many views of one resident source, or of a multi-facet job,
    in one call. `source` is a Source or a list or tuple of them (the facets, composed per pixel as render()
    composes them: args.synopsis); a list of one is that source. `args` gives what the views share (projection,
    size, spline degree, twining); `views` is a sequence of (yaw, pitch, roll) or (yaw, pitch, roll, hfov) in
    degrees, args.hfov applying where a view gives none. Returns (N, H, W, C) float32, view k being render() of args
    with that orientation and hfov, bit for bit: a new numpy array, or `out` (numpy, or a float32
    torch tensor in device memory - of the device the library runs on, which on a host with several is the caller's
    to see to; rows and views may be padded). C defaults to the first facet's channel count. With `out` on the
    device the call is asynchronous on `stream` (a hipStream_t address; None: the library's stream) until sync()."""
    _views_args(args, "render_views")
    views = list(views)
    facets = list(source) if isinstance(source, (list, tuple)) else [source]
    if not facets:
        raise EuError("render_views: no source")
    nch = nchannels or facets[0].fct.nchannels
    shape = (len(views), args.height, args.width, nch)
    if out is None:
        out = np.zeros(shape, np.float32)
    if tuple(out.shape) != shape:
        raise EuError(f"render_views: out has shape {tuple(out.shape)}, expected {shape}")
    optr, row, view, on_device = _frames(out, "out")
    t = args.target(nch)
    arr = _views_struct(args, views)
    st = C.c_void_p(stream) if stream else None
    if len(facets) == 1:
        _check(lib().eu_hip_render_views(C.byref(t), arr, len(views), facets[0].handle, C.c_void_p(optr), row, view,
                                         int(on_device), st))
    else:
        handles = (C.c_void_p * len(facets))(*[s.handle for s in facets])
        _check(lib().eu_hip_render_views_multi(C.byref(t), arr, len(views), handles, len(facets), C.c_void_p(optr),
                                               row, view, int(on_device), st))
    return out


def render_layers(args, sources, nchannels=None, out=None, stream=None):
    """eu_hip_render_layers: many pictures of one geometry in one call. `sources` is a list or tuple of Source that
    share projection, size, field of view, orientation, lens, channel count and spline degree - the eyes of a stereo
    pair, the exposures of a bracket (brighten may differ), passes, frames - and are NOT composed: every one gives a
    frame of its own (render(args, [sources]) is the multi-facet job). Returns (L, H, W, C) float32, layer k being
    render(args, sources[k]) bit for bit: a new numpy array, or `out` (numpy, or a float32 torch tensor in device
    memory; rows and layers may be padded). C defaults to the layers' channel count. With `out` on the device the
    call is asynchronous on `stream` (a hipStream_t address; None: the library's stream) until sync()."""
    _views_args(args, "render_layers")
    if not isinstance(sources, (list, tuple)):
        raise EuError("render_layers: sources is a list or tuple of Source")
    layers = list(sources)
    nch = nchannels or (layers[0].fct.nchannels if layers else 0)
    if not nch:
        raise EuError("render_layers: no layer and no nchannels to shape the result by")
    shape = (len(layers), args.height, args.width, nch)
    if out is None:
        out = np.zeros(shape, np.float32)
    if tuple(out.shape) != shape:
        raise EuError(f"render_layers: out has shape {tuple(out.shape)}, expected {shape}")
    optr, row, layer, on_device = _frames(out, "out")
    t = args.target(nch)
    handles = (C.c_void_p * max(len(layers), 1))(*[s.handle for s in layers])
    _check(lib().eu_hip_render_layers(C.byref(t), handles, len(layers), C.c_void_p(optr), row, layer, int(on_device),
                                      C.c_void_p(stream) if stream else None))
    return out


def view_tables(args, view, source, nchannels=None):
    """eu_hip_view_tables, for tests: the stepper tables of one view as the table kernel of render_views builds
    them and as the host builds them for render(). Returns (col_dev, row_dev, col_host, row_host): columns
    (6, W), rows (H, ROW_FLOATS), float32."""
    _views_args(args, "view_tables")
    t = args.target(nchannels or source.fct.nchannels)
    arr = _views_struct(args, [view])
    cols = [np.zeros((6, args.width), np.float32) for _ in range(2)]
    rows = [np.zeros((args.height, ROW_FLOATS), np.float32) for _ in range(2)]
    _check(lib().eu_hip_view_tables(C.byref(t), arr, source.handle, _ptr(cols[0]), _ptr(rows[0]), _ptr(cols[1]),
                                    _ptr(rows[1])))
    return cols[0], rows[0], cols[1], rows[1]


def listed_tiles():
    """eu_hip_listed_tiles: the wave tiles the last staged launch pair left to the direct-gather kernel"""
    f = lib().eu_hip_listed_tiles
    f.restype = C.c_ulonglong
    return int(f())


def launch_count():
    """eu_hip_launch_count: render kernel launches of single-facet jobs so far"""
    f = lib().eu_hip_launch_count
    f.restype = C.c_ulonglong
    return int(f())


def sync():
    """eu_hip_sync: wait for the library's stream and for what every call so far has left on a caller's stream"""
    _check(lib().eu_hip_sync())


def init_devices(devices):
    """one process, several devices: one slot per entry (the same device may be listed twice)"""
    arr = (C.c_int * len(devices))(*devices)
    _check(lib().eu_hip_init_devices(arr, len(devices)))


def device_slots():
    return lib().eu_hip_device_slots()


def device_strips(args, sources, nchannels=None):
    """the rows eu_hip_render_devices gives every slot for this job: [(begin, end), ...]"""
    if not isinstance(sources, (list, tuple)):
        sources = [sources]
    nch = nchannels or sources[0].fct.nchannels
    t = args.target(nch, 0, None, 0, None)
    n = device_slots()
    b, e = (C.c_int * n)(), (C.c_int * n)()
    arr = (C.c_void_p * len(sources))(*[s.handle for s in sources])
    _check(lib().eu_hip_device_strips(C.byref(t), arr, len(sources), b, e))
    return list(zip(list(b), list(e)))


def render_devices(args, sources, nchannels=None, out=None, out_dev_ptr=None):
    """the whole frame, its rows tiled over the device slots (eu_hip_render_devices): into host memory
    (returned) or, with out_dev_ptr, into device memory of slot 0"""
    if not isinstance(sources, (list, tuple)):
        sources = [sources]
    nch = nchannels or sources[0].fct.nchannels
    t = args.target(nch, 0, None, 0, None)
    rows = t.row_end - t.row_begin
    w = args.out_width
    och = 1 if args.tethered else nch
    arr = (C.c_void_p * len(sources))(*[s.handle for s in sources])
    if out_dev_ptr is not None:
        _check(lib().eu_hip_render_devices(C.byref(t), arr, len(sources), C.c_void_p(out_dev_ptr), w * och * 4, 1))
        return None
    if out is None:
        out = np.zeros((rows, w), np.uint32) if args.tethered else np.zeros((rows, w, och), np.float32)
    _check(lib().eu_hip_render_devices(C.byref(t), arr, len(sources), out.ctypes.data_as(C.c_void_p), w * och * 4, 0))
    return out


def render_timed(args, sources, out_dev_ptr, iters, nchannels=None, row_begin=0,
                 row_end=None, band=None):
    """kernel-only timing with HIP events on the library's stream; the output
    stays in HBM at out_dev_ptr. Returns mean milliseconds per launch."""
    if not isinstance(sources, (list, tuple)):
        sources = [sources]
    nch = nchannels or sources[0].fct.nchannels
    t = args.target(nch, row_begin, row_end, 0, band)
    arr = (C.c_void_p * len(sources))(*[s.handle for s in sources])
    ms = C.c_float()
    och = 1 if args.tethered else nch
    _check(lib().eu_hip_render_timed(C.byref(t), arr, len(sources), C.c_void_p(out_dev_ptr),
                                     args.out_width * och * 4, iters, C.byref(ms)))
    return ms.value


class _hip_dispatch:
    """dispatch_base (envutil_dispatch.h:49-65) for the HIP back-end:
    payload(nchannels, ninputs, projection) runs one render job described by
    the `args` / sources it was bound to and returns 0, like the reference."""

    hwy_target_name = "gfx950"
    hwy_target_str = "HIP/CDNA4"

    def __init__(self):
        self.args = None
        self.sources = None
        self.result = None

    def bind(self, args, sources):
        self.args, self.sources = args, sources
        return self

    def payload(self, nchannels, ninputs, projection):
        a = self.args
        if projection != a.projection:
            raise EuError("payload projection differs from args.projection")
        if (ninputs == 9) != (a.twine_spread is not None):
            raise EuError("ninputs must be 9 with twining and 3 without")
        self.result = render(a, self.sources, nchannels)
        return 0


def get_dispatch():
    return _hip_dispatch()
