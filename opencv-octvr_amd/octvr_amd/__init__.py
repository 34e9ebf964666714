"""Python binding of the MI355X octVR stitching library (include/octvr_hip.h) over ctypes.

Host-side mirror of the reference's octvr API for the stitching path:

* :class:`MapperTemplate`  <- ``vr::MapperTemplate`` (modules/octvr/include/octvr.hpp:47-91)
* :class:`Mapper`          <- ``vr::Mapper``         (modules/octvr/src/mapper.hpp:29-95)

Device buffers are torch tensors on ``cuda:N`` (PyTorch is plumbing here: allocation, streams,
torch.distributed); all arithmetic runs in the hand-written HIP kernels of ``liboctvr_hip.so``.
There is no CPU fallback: importing this module fails loudly when the library is missing.
"""
import ctypes as C
import json as _json
import os

import numpy as np
import torch  # must be imported first: the library then binds to torch's HIP runtime (one per process)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OCTVR_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "liboctvr_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "liboctvr_hip.so not found at %s — build it with `make -C opencv-octvr_amd` or "
        "`python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)

_lib = C.CDLL(LIB_PATH)


# status codes of include/octvr_hip.h
E_INVALID, E_PARSE, E_HIP, E_UNSUPPORTED, E_IO = -1, -2, -3, -4, -5


class OctvrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("octvr error %d: %s" % (code, msg))
        self.code = code


class InputView(C.Structure):
    _fields_ = [("roi_x", C.c_int), ("roi_y", C.c_int), ("roi_w", C.c_int), ("roi_h", C.c_int),
                ("map1", C.c_void_p), ("map2", C.c_void_p), ("mask", C.c_void_p), ("seam_mask", C.c_void_p),
                ("vignette", C.c_void_p), ("vignette_w", C.c_int), ("vignette_h", C.c_int)]


def _check(rc):
    if rc != 0:
        raise OctvrError(rc, _lib.octvr_last_error().decode())


_lib.octvr_last_error.restype = C.c_char_p
_VP = C.c_void_p
_lib.octvr_rig_create_json.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]
_lib.octvr_rig_load_dat.argtypes = [C.c_char_p, C.POINTER(_VP)]
_lib.octvr_rig_dump_dat.argtypes = [_VP, C.c_char_p]
_lib.octvr_rig_create_masks.argtypes = [_VP, C.c_int]
_lib.octvr_rig_create_from_arrays.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(_VP),
                                              C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP)]
_lib.octvr_rig_num_inputs.argtypes = [_VP, C.POINTER(C.c_int)]
_lib.octvr_rig_out_size.argtypes = [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]
_lib.octvr_rig_get_input.argtypes = [_VP, C.c_int, C.POINTER(InputView)]
_lib.octvr_rig_num_overlays.argtypes = [_VP, C.POINTER(C.c_int)]
_lib.octvr_rig_get_overlay.argtypes = [_VP, C.c_int, C.POINTER(InputView)]
_lib.octvr_rig_morph_controlpoints.argtypes = [_VP, C.c_char_p, C.POINTER(C.c_int)]
_lib.octvr_rig_get_triangles.argtypes = [_VP, C.c_int, _VP, _VP, C.c_int, C.POINTER(C.c_int)]
_lib.octvr_rig_set_vignette.argtypes = [_VP, C.c_int, C.c_int, _VP, C.c_int, C.c_int]
_lib.octvr_rig_destroy.argtypes = [_VP]
_lib.octvr_rig_destroy.restype = None
_lib.octvr_mapper_create.argtypes = [_VP, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.POINTER(_VP)]
if hasattr(_lib, "octvr_mapper_create_ex"):
    _lib.octvr_mapper_create_ex.argtypes = [_VP, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                            C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]
REMAP_TEXTURE = 1  # octvr_hip.h OCTVR_REMAP_TEXTURE
_lib.octvr_mapper_stitch_batch.argtypes = [_VP, C.c_int, C.POINTER(_VP), C.POINTER(C.c_size_t), C.POINTER(_VP),
                                           C.c_size_t, _VP, _VP]
_lib.octvr_mapper_stitch_yuv420p.argtypes = [_VP, C.POINTER(_VP), C.POINTER(C.c_size_t), _VP, C.c_size_t,
                                             C.POINTER(C.c_double), C.c_int, _VP]
_lib.octvr_mapper_stitch_preview.argtypes = [_VP, C.POINTER(_VP), C.POINTER(C.c_size_t), _VP, C.c_size_t, _VP, C.c_int,
                                             C.c_int, C.c_size_t, C.POINTER(C.c_double), C.c_int, _VP]
if hasattr(_lib, "octvr_mapper_prepare_preview"):  # (absent from older libraries OCTVR_HIP_LIB may select for an A/B)
    _lib.octvr_mapper_prepare_preview.argtypes = [_VP, _VP, C.c_int, C.c_int]
TENSOR_U8, TENSOR_F16, TENSOR_F32 = 0, 1, 2  # OCTVR_TENSOR_*


class TensorOut(C.Structure):
    """octvr_tensor_out: three planes of u8 / f16 / f32 on the device, strides in elements."""
    _fields_ = [("dev", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("dtype", C.c_int), ("bgr", C.c_int),
                ("row_stride", C.c_size_t), ("plane_stride", C.c_size_t), ("scale", C.c_float * 3),
                ("bias", C.c_float * 3)]


if hasattr(_lib, "octvr_mapper_stitch_tensor"):
    _lib.octvr_mapper_stitch_tensor.argtypes = [_VP, C.POINTER(_VP), C.POINTER(C.c_size_t), _VP, C.c_size_t,
                                                C.POINTER(TensorOut), C.POINTER(C.c_double), C.c_int, _VP]
_lib.octvr_mapper_gains.argtypes = [_VP, C.POINTER(C.c_double), C.c_int]
_lib.octvr_mapper_set_frames_in_flight.argtypes = [_VP, C.c_int]
if hasattr(_lib, "octvr_mapper_set_pixel_formats"):  # (absent from libraries built before NV12: scripts/ab.sh variants)
    _lib.octvr_mapper_set_pixel_formats.argtypes = [_VP, C.c_int, C.c_int]
    _lib.octvr_mapper_pixel_formats.argtypes = [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]
_lib.octvr_mapper_traffic.argtypes = [_VP, C.POINTER(C.c_double)]
_lib.octvr_mapper_set_timing.argtypes = [_VP, C.c_int]
_lib.octvr_mapper_kernel_time.argtypes = [_VP, C.POINTER(C.c_double), C.POINTER(C.c_int)]
_lib.octvr_mapper_kernel_busy.argtypes = [_VP, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
_lib.octvr_mapper_kernel_intervals.argtypes = [_VP, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int,
                                               C.POINTER(C.c_int)]
_lib.octvr_rig_lut_recomputed.argtypes = [_VP, C.c_int, C.POINTER(C.c_uint64)]
_lib.octvr_debug_project_f64.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _VP, _VP, _VP]
_lib.octvr_interval_union.argtypes = [_VP, _VP, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
_lib.octvr_fastmapper_traffic.argtypes = [_VP, C.POINTER(C.c_double)]
_lib.octvr_mapper_info.argtypes = [_VP, C.c_char_p, C.c_size_t]
_lib.octvr_mapper_destroy.argtypes = [_VP]
_lib.octvr_mapper_destroy.restype = None
_lib.octvr_async_create.argtypes = [C.POINTER(_VP), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                    C.POINTER(_VP)]
if hasattr(_lib, "octvr_async_create_ex"):
    _lib.octvr_async_create_ex.argtypes = [C.POINTER(_VP), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                           C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                           C.POINTER(C.c_double), C.c_int, C.POINTER(_VP)]
_lib.octvr_async_create_preview.argtypes = [C.POINTER(_VP), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                            C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int),
                                            C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int,
                                            C.POINTER(_VP)]


class PreviewDataHeader(C.Structure):
    """vr::PreviewDataHeader (octvr.hpp:97-101) = octvr_preview_header."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("step", C.c_int), ("fps", C.c_double)]


PREVIEW_SINK = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(PreviewDataHeader))
_lib.octvr_async_pop_preview.argtypes = [_VP, _VP, C.c_size_t, C.POINTER(PreviewDataHeader)]
_lib.octvr_async_set_preview_sink.argtypes = [_VP, PREVIEW_SINK, _VP]
_lib.octvr_async_info.argtypes = [_VP, C.c_char_p, C.c_size_t]
_lib.octvr_async_register_output.argtypes = [_VP, C.POINTER(_VP), C.POINTER(C.c_size_t)]
_lib.octvr_async_unregister_output.argtypes = [_VP, C.POINTER(_VP)]
_lib.octvr_async_push.argtypes = [_VP, C.POINTER(_VP), C.POINTER(C.c_size_t), C.POINTER(_VP), C.POINTER(C.c_size_t)]
if hasattr(_lib, "octvr_async_push_device"):  # (absent from older libraries OCTVR_HIP_LIB may select for an A/B)
    _lib.octvr_async_push_device.argtypes = [_VP, C.POINTER(_VP), C.POINTER(C.c_size_t), _VP, C.c_size_t, _VP]
_lib.octvr_async_pop.argtypes = [_VP]
_lib.octvr_async_pending.argtypes = [_VP, C.POINTER(C.c_int)]
if hasattr(_lib, "octvr_async_set_pixel_formats"):  # (absent from older libraries OCTVR_HIP_LIB may select for an A/B)
    _lib.octvr_async_set_pixel_formats.argtypes = [_VP, C.c_int, C.c_int]
    _lib.octvr_async_pixel_formats.argtypes = [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]
if hasattr(_lib, "octvr_async_set_output_format"):  # (absent from older libraries OCTVR_HIP_LIB may select for an A/B)
    _lib.octvr_async_set_output_format.argtypes = [_VP, C.c_int]
_lib.octvr_async_destroy.argtypes = [_VP]
_lib.octvr_async_destroy.restype = None
_lib.octvr_fill_poly_u8.argtypes = [_VP, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_uint8]
_lib.octvr_png_decode_rgb.argtypes = [C.c_char_p, C.c_size_t, _VP, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
_lib.octvr_fastmapper_create.argtypes = [_VP, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_VP)]
_lib.octvr_fastmapper_stitch_nv12.argtypes = [_VP, C.POINTER(_VP), C.POINTER(C.c_size_t), _VP, C.c_size_t, _VP]
_lib.octvr_fastmapper_stitch_nv12_batch.argtypes = [_VP, C.c_int, C.POINTER(_VP), C.POINTER(C.c_size_t),
                                                    C.POINTER(_VP), C.c_size_t, _VP]
_lib.octvr_fastmapper_traffic_parts.argtypes = [_VP, C.POINTER(C.c_double), C.POINTER(C.c_double)]
_lib.octvr_mapper_traffic_parts.argtypes = [_VP, C.POINTER(C.c_double), C.POINTER(C.c_double)]
_lib.octvr_fastmapper_destroy.argtypes = [_VP]
_lib.octvr_fastmapper_destroy.restype = None
# self-test hooks (absent from older builds that OCTVR_HIP_LIB may select for an A/B)
if hasattr(_lib, "octvr_debug_json_number"):
    _lib.octvr_debug_json_number.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_double)]
if hasattr(_lib, "octvr_debug_tiled_lut_info"):
    _lib.octvr_debug_tiled_lut_info.argtypes = [_VP, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                                C.c_char_p, C.c_size_t]
if hasattr(_lib, "octvr_debug_entry_pack"):
    _lib.octvr_debug_entry_pack.argtypes = [_VP, C.c_int, C.c_uint32, _VP, _VP, _VP]
if hasattr(_lib, "octvr_debug_fastmapper_audit"):
    _lib.octvr_debug_fastmapper_audit.argtypes = [_VP, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                                  C.c_int, C.c_char_p, C.c_size_t]
if hasattr(_lib, "octvr_debug_gain_plan"):
    _lib.octvr_debug_gain_plan.argtypes = [_VP, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, _VP, _VP,
                                           C.c_size_t, C.POINTER(C.c_size_t)]
if hasattr(_lib, "octvr_debug_pack_runs"):
    _lib.octvr_debug_pack_runs.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _VP, C.c_int, C.POINTER(_VP),
                                           C.POINTER(C.c_size_t), C.c_int, _VP, C.c_size_t, _VP, C.POINTER(C.c_size_t)]
if hasattr(_lib, "octvr_debug_mapper_uyvy_runs"):
    _lib.octvr_debug_mapper_uyvy_runs.argtypes = [_VP, _VP, C.c_size_t, C.POINTER(C.c_size_t)]
if hasattr(_lib, "octvr_debug_worker_failure"):
    _lib.octvr_debug_worker_failure.argtypes = [C.c_int, C.c_int]
if hasattr(_lib, "octvr_debug_gain_solve"):
    _lib.octvr_debug_gain_solve.argtypes = [_VP, _VP, C.c_int, C.c_int, C.c_int, _VP, _VP]
_lib.octvr_remap_u8.argtypes = [_VP, C.c_int, C.c_int, C.c_size_t, C.c_int, _VP, _VP, C.c_int, C.c_int, C.c_size_t,
                                C.c_float, C.c_float, _VP, C.c_size_t, _VP]


def lib():
    return _lib


def abi_version():
    return _lib.octvr_abi_version()


def debug_project_f64(rig_json, out_w, out_h, input, device=0, where=0):
    """(x, y, fragile) — the FP64 projection of every output pixel for one input of a JSON rig, on the
    GPU (where=0; fragile = the LUT guard's verdict) or on the host with glibc (where=1; fragile None)
    (octvr_debug_project_f64)."""
    import numpy as _np
    x = _np.empty((out_h, out_w), _np.float64)
    y = _np.empty((out_h, out_w), _np.float64)
    f = _np.zeros((out_h, out_w), _np.uint8)
    _check(_lib.octvr_debug_project_f64(rig_json.encode() if isinstance(rig_json, str) else rig_json, out_w, out_h,
                                        int(input), int(device), int(where), x.ctypes.data_as(_VP),
                                        y.ctypes.data_as(_VP), f.ctypes.data_as(_VP)))
    return x, y, (f if where == 0 else None)


def debug_tiled_lut_info(mt, in_sizes, remap="remap"):
    """The blend = 0 composite's tiled LUT built on the host (octvr_debug_tiled_lut_info; no GPU), with its
    staged-group coverage check: a dict of items, wide tiles, staged / box pixels, bytes, histograms."""
    n = len(in_sizes)
    w = (C.c_int * n)(*[s[0] for s in in_sizes])
    h = (C.c_int * n)(*[s[1] for s in in_sizes])
    buf = C.create_string_buffer(4096)
    _check(_lib.octvr_debug_tiled_lut_info(mt._h, n, w, h, REMAP_TEXTURE if remap == "texture" else 0, buf, len(buf)))
    import json as _json
    return _json.loads(buf.value.decode())


def debug_entry_pack(entries, stride):
    """(ok, records, unpacked) of quads of four 4-byte tiled entries (an (n, 4) uint32 array) of an item of LDS
    row stride `stride`: whether each quad qualifies for an 8-byte quad record, the record, and the entries
    it decodes back to (octvr_debug_entry_pack; no GPU)."""
    import numpy as _np
    e = _np.ascontiguousarray(entries, _np.uint32).reshape(-1, 4)
    n = e.shape[0]
    rec = _np.zeros(n, _np.uint64)
    ok = _np.zeros(n, _np.uint8)
    un = _np.zeros((n, 4), _np.uint32)
    _check(_lib.octvr_debug_entry_pack(e.ctypes.data_as(_VP), n, int(stride), rec.ctypes.data_as(_VP),
                                       ok.ctypes.data_as(_VP), un.ctypes.data_as(_VP)))
    return ok.astype(bool), rec, un


def _plane_args(plane_sets):
    """(pointers, pitches, kept arrays) of (Y, U, V) or (Y, UV[, None]) plane tuples, three entries per set; a
    missing or None third plane is a NULL pointer with pitch 0 (NV12: octvr_async_set_pixel_formats)."""
    planes = []
    for tri in plane_sets:
        tri = list(tri)
        if len(tri) not in (1, 2, 3):
            raise ValueError("a plane set is (Y, U, V), (Y, UV) for an NV12 side or (UYVY,) for a packed 4:2:2 input")
        tri += [None] * (3 - len(tri))
        for k, p in enumerate(tri):
            if p is not None and p.dtype == np.uint16 and p.ndim == 2 and p.strides[1] == 2:
                p = tri[k] = p.view(np.uint8)  # a plane of 16-bit words (the 10-bit formats) as its bytes
            if p is not None:
                assert p.dtype == np.uint8 and p.ndim == 2 and p.strides[1] == 1, \
                    "uint8 2-D planes with unit column stride"
            planes.append(p)
    ptr = (_VP * len(planes))(*[None if p is None else p.ctypes.data for p in planes])
    pitch = (C.c_size_t * len(planes))(*[0 if p is None else p.strides[0] for p in planes])
    return ptr, pitch, planes


def debug_pack_runs(in_sizes, runs, planes, fmt="yuv420p"):
    """(packed, sizes): the AsyncMultiMapper copy-in's packing (octvr_debug_pack_runs; no GPU) of `runs`, rows
    of (camera, row pair, first group, groups), from per-camera plane tuples laid out as push() takes them
    for `fmt` — the packed bytes back to back and each run's size."""
    n = len(in_sizes)
    w = (C.c_int * n)(*[s[0] for s in in_sizes])
    h = (C.c_int * n)(*[s[1] for s in in_sizes])
    r = np.ascontiguousarray(np.asarray(runs, np.uint32).reshape(-1, 4))
    ptr, pitch, keep = _plane_args(planes)
    cap = int(sum(8 * 8 * int(x[3]) for x in r)) + 8
    packed = np.full(cap, 0x5A, np.uint8)
    sizes = np.zeros(len(r), np.uintp)
    total = C.c_size_t()
    _check(_lib.octvr_debug_pack_runs(n, w, h, r.ctypes.data_as(_VP), len(r), ptr, pitch, _pix_value(fmt),
                                      packed.ctypes.data_as(_VP), cap, sizes.ctypes.data_as(_VP), C.byref(total)))
    assert (packed[total.value:] == 0x5A).all()
    return packed[:total.value].copy(), sizes.astype(np.int64)


def debug_mapper_uyvy_runs(mapper):
    """The footprint runs a "uyvy422"-input Mapper's unpack launch converts: an (n, 4) array of (camera, row
    pair, first group, groups) (octvr_debug_mapper_uyvy_runs)."""
    n = C.c_size_t()
    _check(_lib.octvr_debug_mapper_uyvy_runs(mapper._h, None, 0, C.byref(n)))
    runs = np.zeros((n.value, 4), np.uint32)
    _check(_lib.octvr_debug_mapper_uyvy_runs(mapper._h, runs.ctypes.data_as(_VP), n.value, C.byref(n)))
    return runs


def debug_worker_failure(n_threads, failing):
    """Run the host build's worker-thread helper with thread `failing` raising (octvr_debug_worker_failure;
    no GPU): raises OctvrError with the worker's message, as a failing tiler / seam / audit worker does."""
    _check(_lib.octvr_debug_worker_failure(int(n_threads), int(failing)))


def debug_gain_plan(mt, in_sizes, remap="remap"):
    """(entries, partners): the gain feed's samples as the mapper lays them out (octvr_debug_gain_plan; no
    GPU) — entries an (n, 2) uint32 array of (xy, code), partners a uint16 array."""
    import numpy as _np
    n = len(in_sizes)
    w = (C.c_int * n)(*[s[0] for s in in_sizes])
    h = (C.c_int * n)(*[s[1] for s in in_sizes])
    fl = REMAP_TEXTURE if remap == "texture" else 0
    cnt = C.c_size_t()
    _check(_lib.octvr_debug_gain_plan(mt._h, n, w, h, fl, None, None, 0, C.byref(cnt)))
    e = _np.zeros((cnt.value, 2), _np.uint32)
    p = _np.zeros(cnt.value, _np.uint16)
    _check(_lib.octvr_debug_gain_plan(mt._h, n, w, h, fl, e.ctypes.data, p.ctypes.data, cnt.value, C.byref(cnt)))
    return e, p


def debug_gain_solve(A, b, lean=False):
    """(x, ok) of `count` n x n systems (A: (count, n, n), b: (count, n), float64) through the gain feed's
    device solver, one workgroup each (octvr_debug_gain_solve): lean=False the full feed's choice of solver,
    True the lean feed's.  ok: bool per system; x rows are zero where it is False."""
    import numpy as _np
    A = _np.ascontiguousarray(A, _np.float64)
    b = _np.ascontiguousarray(b, _np.float64)
    count, n = b.shape
    assert A.shape == (count, n, n)
    x = _np.zeros((count, n), _np.float64)
    ok = _np.zeros(count, _np.int32)
    _check(_lib.octvr_debug_gain_solve(A.ctypes.data_as(_VP), b.ctypes.data_as(_VP), n, count, int(bool(lean)),
                                       x.ctypes.data_as(_VP), ok.ctypes.data_as(_VP)))
    return x, ok.astype(bool)


def debug_json_number(text, exact=True):
    """The first number of a JSON document as the rig-config reader parses it (octvr_debug_json_number):
    exact=True correctly rounded (OCTVR_JSON_EXACT), False with rapidjson's rules."""
    v = C.c_double()
    _check(_lib.octvr_debug_json_number(text.encode(), 1 if exact else 0, C.byref(v)))
    return v.value


def debug_fastmapper_audit(mt, in_sizes, wide=False, pitch_pad=0):
    """(ok, report): the host replay of every index the FastMapper kernels derive for this template and
    these input sizes, in the compact or (wide=True) 8-byte entry format (octvr_debug_fastmapper_audit;
    no GPU).  report: per plane ("y", "uv") the counts and the first violation.  Every input frame is taken at
    pitch w + pitch_pad; addresses are replayed relative to the frame's base, so a base that is not 4-byte
    aligned is covered by the GPU test only (tests/test_gpu_fastmapper_layouts.py)."""
    n = len(in_sizes)
    w = (C.c_int * n)(*[s[0] for s in in_sizes])
    h = (C.c_int * n)(*[s[1] for s in in_sizes])
    buf = C.create_string_buffer(4096)
    rc = _lib.octvr_debug_fastmapper_audit(mt._h, n, w, h, int(bool(wide)), int(pitch_pad), buf, len(buf))
    import json as _json
    if not buf.value:  # the plan itself failed (bad arguments): no report
        _check(rc)
    return rc == 0, _json.loads(buf.value.decode())


def interval_union(starts, ends):
    """(summed lengths, length of the union) of the intervals [starts[k], ends[k]]
    (octvr_interval_union: the arithmetic of Mapper.kernel_busy)."""
    import numpy as _np
    a = _np.ascontiguousarray(starts, _np.float64)
    b = _np.ascontiguousarray(ends, _np.float64)
    sp, bu = C.c_double(), C.c_double()
    _check(_lib.octvr_interval_union(a.ctypes.data_as(_VP), b.ctypes.data_as(_VP), len(a), C.byref(sp), C.byref(bu)))
    return sp.value, bu.value


def _stream_ptr(stream):
    if isinstance(stream, C.c_void_p):
        return stream
    if stream is None:
        stream = torch.cuda.current_stream()
    return C.c_void_p(stream.cuda_stream)


class MapperTemplate:
    """vr::MapperTemplate: JSON rig (LUT built on the GPU) or a VRv11 .dat file."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)

    @classmethod
    def from_json(cls, rig, out_w, out_h, use_roi=True, device=0):
        text = rig if isinstance(rig, str) else _json.dumps(rig)
        h = _VP()
        _check(_lib.octvr_rig_create_json(text.encode(), out_w, out_h, int(use_roi), device, C.byref(h)))
        return cls(h.value)

    @classmethod
    def load(cls, path):
        h = _VP()
        _check(_lib.octvr_rig_load_dat(os.fsencode(path), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_arrays(cls, out_w, out_h, rois, map1s, map2s, masks, seams=None):
        n = len(rois)
        map1s = [np.ascontiguousarray(a, np.float32) for a in map1s]
        map2s = [np.ascontiguousarray(a, np.float32) for a in map2s]
        masks = [np.ascontiguousarray(a, np.uint8) for a in masks]
        r = (C.c_int * (4 * n))(*[int(v) for roi in rois for v in roi])
        p1 = (_VP * n)(*[a.ctypes.data for a in map1s])
        p2 = (_VP * n)(*[a.ctypes.data for a in map2s])
        pm = (_VP * n)(*[a.ctypes.data for a in masks])
        ps = None
        if seams is not None:
            seams = [np.ascontiguousarray(a, np.uint8) for a in seams]
            ps = (_VP * n)(*[a.ctypes.data for a in seams])
        h = _VP()
        _check(_lib.octvr_rig_create_from_arrays(out_w, out_h, n, r, p1, p2, pm, ps, C.byref(h)))
        return cls(h.value)

    def dump(self, path):
        """MapperTemplate::dump: VRv11 file (creates the seam masks first if there are none)."""
        _check(_lib.octvr_rig_dump_dat(self._h, os.fsencode(path)))

    def lut_recomputed(self, i):
        """Output pixels of input i whose projection the GPU LUT build left to the host (glibc)."""
        n = C.c_uint64()
        _check(_lib.octvr_rig_lut_recomputed(self._h, i, C.byref(n)))
        return n.value

    def create_masks(self, device=0):
        """MapperTemplate::create_masks(): L2 distance seams (resizes on `device`)."""
        _check(_lib.octvr_rig_create_masks(self._h, device))

    def morph_controlpoints(self, control_points):
        """MapperTemplate::morph_controlpoints (template_morph.cpp:69-237): control_points is the rig
        JSON's "control_points" list of [n0, n1, x0, y0, x1, y1].  Returns the number kept."""
        text = control_points if isinstance(control_points, str) else _json.dumps(control_points)
        k = C.c_int()
        _check(_lib.octvr_rig_morph_controlpoints(self._h, text.encode(), C.byref(k)))
        return k.value

    def triangles(self, i):
        """inputs[i].src_triangles, dst_triangles of the last morph: two (n, 6) float32 arrays."""
        n = C.c_int()
        _check(_lib.octvr_rig_get_triangles(self._h, i, None, None, 0, C.byref(n)))
        src = np.zeros((n.value, 6), np.float32)
        dst = np.zeros((n.value, 6), np.float32)
        _check(_lib.octvr_rig_get_triangles(self._h, i, src.ctypes.data, dst.ctypes.data, n.value, C.byref(n)))
        return src, dst

    @property
    def out_size(self):
        w, h = C.c_int(), C.c_int()
        _check(_lib.octvr_rig_out_size(self._h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def __len__(self):
        n = C.c_int()
        _check(_lib.octvr_rig_num_inputs(self._h, C.byref(n)))
        return n.value

    @property
    def num_overlays(self):
        n = C.c_int()
        _check(_lib.octvr_rig_num_overlays(self._h, C.byref(n)))
        return n.value

    def overlay(self, i):
        """Overlay input i (MapperTemplate::overlay_inputs): (roi, map1, map2, mask, None)."""
        return self.input(i, _overlay=True)

    def input(self, i, _overlay=False):
        """(roi, map1, map2, mask, seam_mask) as numpy copies."""
        v = InputView()
        _check((_lib.octvr_rig_get_overlay if _overlay else _lib.octvr_rig_get_input)(self._h, i, C.byref(v)))
        k = v.roi_w * v.roi_h
        shape = (v.roi_h, v.roi_w)

        def arr(ptr, ctype, dtype):
            if not ptr:
                return None
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(k,)).astype(dtype).reshape(shape)

        return ((v.roi_x, v.roi_y, v.roi_w, v.roi_h), arr(v.map1, C.c_float, np.float32),
                arr(v.map2, C.c_float, np.float32), arr(v.mask, C.c_uint8, np.uint8),
                arr(v.seam_mask, C.c_uint8, np.uint8))

    def vignette(self, i):
        """The input's vignette map (Vignette::getMap, vignette.cpp:39-54) or None."""
        v = InputView()
        _check(_lib.octvr_rig_get_input(self._h, i, C.byref(v)))
        if not v.vignette:
            return None
        k = v.vignette_w * v.vignette_h
        return np.ctypeslib.as_array(C.cast(v.vignette, C.POINTER(C.c_float)), shape=(k,)).copy().reshape(
            v.vignette_h, v.vignette_w)

    def set_vignette(self, i, gain_map):
        """Sets input i's vignette map (octvr_rig_set_vignette): a 2-D float32 array of gains, resized to the
        camera's size by the mappers created afterwards; None removes it."""
        if gain_map is None:
            _check(_lib.octvr_rig_set_vignette(self._h, int(i), 0, None, 0, 0))
            return
        a = np.ascontiguousarray(gain_map, np.float32)
        assert a.ndim == 2
        _check(_lib.octvr_rig_set_vignette(self._h, int(i), 0, a.ctypes.data_as(_VP), a.shape[1], a.shape[0]))

    def close(self):
        if self._h and self._h.value:
            _lib.octvr_rig_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FrameRefs:
    """A frame set's device pointers and pitches marshalled once (Mapper.frame_refs), for callers that
    stitch the same buffers repeatedly (a capture ring): stitch() then skips the per-call ctypes work."""
    __slots__ = ("tensors", "ptrs", "pitches", "n")

    def __init__(self, tensors):
        self.tensors = list(tensors)  # kept alive while the references are in use
        self.n = len(self.tensors)
        self.ptrs = (_VP * self.n)(*[t.data_ptr() for t in self.tensors])
        self.pitches = (C.c_size_t * self.n)(*[t.stride(0) for t in self.tensors])


class BatchRefs:
    """Several frame sets' device pointers and their outputs marshalled once (Mapper.batch_refs)."""
    __slots__ = ("keep", "ptrs", "pitches", "outs", "out_pitch", "nf")

    def __init__(self, frame_sets, outputs):
        refs = [fs if isinstance(fs, FrameRefs) else FrameRefs(fs) for fs in frame_sets]
        self.nf = len(refs)
        assert len(outputs) == self.nf, "one output per frame set"
        self.keep = (refs, list(outputs))
        ptrs = [p for r in refs for p in r.ptrs]
        pitches = [p for r in refs for p in r.pitches]
        self.ptrs = (_VP * len(ptrs))(*ptrs)
        self.pitches = (C.c_size_t * len(pitches))(*pitches)
        self.outs = (_VP * self.nf)(*[o.data_ptr() for o in outputs])
        self.out_pitch = outputs[0].stride(0)
        assert all(o.stride(0) == self.out_pitch for o in outputs), "the outputs of a batch share one pitch"


PIX_YUV420P, PIX_NV12, PIX_UYVY422 = 0, 1, 16  # OCTVR_PIX_*
PIX_YUYV422, PIX_YUV422P, PIX_NV16 = 17, 18, 19  # the other 8-bit 4:2:2 capture layouts
PIX_P010, PIX_YUV420P10, PIX_P210, PIX_YUV422P10 = 32, 33, 34, 35  # 10-bit samples in 16-bit little-endian words
PIX_V210 = 48  # 10-bit 4:2:2, three samples a 32-bit word, six pixels a 16-byte block (SDI capture, the v210 codec)
PIX_NAMES = ("yuv420p", "nv12")  # the 4:2:0 layouts, by value
_PIX_BY_NAME = {"yuv420p": PIX_YUV420P, "nv12": PIX_NV12, "uyvy422": PIX_UYVY422, "yuyv422": PIX_YUYV422,
                "yuv422p": PIX_YUV422P, "nv16": PIX_NV16, "p010": PIX_P010, "yuv420p10": PIX_YUV420P10,
                "p210": PIX_P210, "yuv422p10": PIX_YUV422P10, "v210": PIX_V210}
_PIX_10BIT = (PIX_P010, PIX_YUV420P10, PIX_P210, PIX_YUV422P10)
_PIX_BY_VALUE = {v: k for k, v in _PIX_BY_NAME.items()}


def _pix_value(fmt):
    if isinstance(fmt, str):
        if fmt.lower() not in _PIX_BY_NAME:
            raise ValueError("pixel format must be 'yuv420p', 'nv12', 'uyvy422', 'yuyv422', 'yuv422p', 'nv16', "
                             "'p010', 'yuv420p10', 'p210', 'yuv422p10' or 'v210'")
        return _PIX_BY_NAME[fmt.lower()]
    return int(fmt)  # the library rejects unknown values (OCTVR_E_INVALID)


def v210_row_bytes(w):
    """Bytes of a w-pixel row of a "v210" frame: 16-byte blocks of six pixels, the row padded to 48 pixels."""
    return 128 * ((int(w) + 47) // 48)


def frame_shape(fmt, w, h):
    """(rows, columns) of a w x h frame in `fmt`: (3h/2, w) for the 4:2:0 layouts, (h, 2w) for "uyvy422" and
    "yuyv422", (2h, w) for "yuv422p" and "nv16".  The 10-bit layouts in bytes (a sample is a 16-bit little-endian
    word): (3h/2, 2w) for "p010" and "yuv420p10", (2h, 2w) for "p210" and "yuv422p10"; (h, v210_row_bytes(w)) for
    "v210"."""
    v = _pix_value(fmt)
    if v == PIX_V210:
        return (int(h), v210_row_bytes(w))
    if v in (PIX_P010, PIX_YUV420P10):
        return (int(h) * 3 // 2, 2 * int(w))
    if v in (PIX_P210, PIX_YUV422P10):
        return (2 * int(h), 2 * int(w))
    if v in (PIX_UYVY422, PIX_YUYV422):
        return (int(h), 2 * int(w))
    if v in (PIX_YUV422P, PIX_NV16):
        return (2 * int(h), int(w))
    return (int(h) * 3 // 2, int(w))


def plane_shapes(fmt, w, h):
    """[(rows, bytes per row)] of the host planes of a w x h frame in `fmt`, as AsyncMultiMapper.push takes them: one
    packed plane; Y and the U,V plane; or Y, U and V (each half a row's bytes wide)."""
    v = _pix_value(fmt)
    w, h, S = int(w), int(h), 2 if v in _PIX_10BIT else 1
    if v in (PIX_UYVY422, PIX_YUYV422):
        return [(h, 2 * w)]
    if v == PIX_V210:
        return [(h, v210_row_bytes(w))]
    ch = h // 2 if v in (PIX_YUV420P, PIX_NV12, PIX_P010, PIX_YUV420P10) else h
    if v in (PIX_NV12, PIX_NV16, PIX_P010, PIX_P210):
        return [(h, S * w), (ch, S * w)]
    return [(h, S * w), (ch, S * w // 2), (ch, S * w // 2)]


def _chroma_frame(frame, w, h):
    f = np.asarray(frame)
    w, h = int(w), int(h)
    if w <= 0 or h <= 0 or (w & 1) or (h & 1):
        raise ValueError("4:2:0 frames have even width and height")
    if f.ndim != 2 or f.dtype != np.uint8 or f.shape[0] != h * 3 // 2 or f.shape[1] < w:
        raise ValueError("expected a uint8 frame of 3h/2 rows and at least w columns")
    return f, w, h


def nv12_from_yuv420p(frame, w, h):
    """The NV12 frame (h rows of Y, then h/2 rows of U,V byte pairs) of a "Y over [U|V]" frame (h rows of Y,
    then h/2 rows with U in bytes [0, w/2) and V in [w/2, w)): a new 3h/2 x w array.  Columns of `frame` past
    w (a pitch) are dropped."""
    f, w, h = _chroma_frame(frame, w, h)
    out = np.array(f[:, :w], dtype=np.uint8, order="C")
    out[h:, 0::2] = f[h:, :w // 2]
    out[h:, 1::2] = f[h:, w // 2:w]
    return out


def yuv420p_from_nv12(frame, w, h):
    """The inverse of nv12_from_yuv420p."""
    f, w, h = _chroma_frame(frame, w, h)
    out = np.array(f[:, :w], dtype=np.uint8, order="C")
    out[h:, :w // 2] = f[h:, 0:w:2]
    out[h:, w // 2:] = f[h:, 1:w:2]
    return out


def uyvy422_from_yuv420p(frame, w, h):
    """The packed UYVY 4:2:2 frame (h rows of 2w bytes, U0 Y0 V0 Y1 per pixel pair) of a "Y over [U|V]" frame by
    the library's output rule: packed rows 2r and 2r + 1 both carry chroma row r, luma is copied."""
    f, w, h = _chroma_frame(frame, w, h)
    out = np.empty((h, 2 * w), np.uint8)
    out[:, 1::2] = f[:h, :w]
    out[:, 0::4] = np.repeat(f[h:, :w // 2], 2, axis=0)
    out[:, 2::4] = np.repeat(f[h:, w // 2:w], 2, axis=0)
    return out


def yuv420p_from_uyvy422(frame, w, h):
    """The "Y over [U|V]" frame of a packed UYVY 4:2:2 frame (h rows, at least 2w columns) by the library's
    input rule: chroma row r is (c[2r] + c[2r + 1] + 1) >> 1 per byte of the packed rows 2r and 2r + 1, luma is
    copied."""
    f = np.asarray(frame)
    w, h = int(w), int(h)
    if w <= 0 or h <= 0 or (w & 1) or (h & 1):
        raise ValueError("4:2:2 frames have even width and height")
    if f.ndim != 2 or f.dtype != np.uint8 or f.shape[0] != h or f.shape[1] < 2 * w:
        raise ValueError("expected a uint8 frame of h rows and at least 2w columns")
    out = np.empty((h * 3 // 2, w), np.uint8)
    out[:h] = f[:, 1:2 * w:2]
    c = f[:, 0:2 * w:2].astype(np.uint16)  # U,V pairs of every packed row
    avg = ((c[0::2] + c[1::2] + 1) >> 1).astype(np.uint8)
    out[h:, :w // 2] = avg[:, 0::2]
    out[h:, w // 2:] = avg[:, 1::2]
    return out


def yuv422_from_yuv420p(fmt, frame, w, h):
    """The frame in the 4:2:2 layout `fmt` ("uyvy422", "yuyv422", "yuv422p", "nv16" or the PIX_* value; shape
    frame_shape(fmt, w, h)) of a "Y over [U|V]" frame by the library's output rule: chroma rows 2r and 2r + 1 both
    carry chroma row r, luma is copied."""
    v = _pix_value(fmt)
    if v == PIX_UYVY422:
        return uyvy422_from_yuv420p(frame, w, h)
    if v not in (PIX_YUYV422, PIX_YUV422P, PIX_NV16):
        raise ValueError("not a 4:2:2 layout")
    f, w, h = _chroma_frame(frame, w, h)
    u = np.repeat(f[h:, :w // 2], 2, axis=0)
    vv = np.repeat(f[h:, w // 2:w], 2, axis=0)
    out = np.empty(frame_shape(v, w, h), np.uint8)
    if v == PIX_YUYV422:
        out[:, 0::2] = f[:h, :w]
        out[:, 1::4] = u
        out[:, 3::4] = vv
        return out
    out[:h] = f[:h, :w]
    if v == PIX_YUV422P:
        out[h:, :w // 2] = u
        out[h:, w // 2:] = vv
    else:
        out[h:, 0::2] = u
        out[h:, 1::2] = vv
    return out


def yuv422_planes(fmt, frame, w, h):
    """(luma, U, V) of a frame in the 4:2:2 layout `fmt`, each as an array of h rows (U and V w/2 columns wide);
    columns of `frame` past a row's width (a pitch) are dropped."""
    v = _pix_value(fmt)
    f = np.asarray(frame)
    w, h = int(w), int(h)
    if w <= 0 or h <= 0 or (w & 1) or (h & 1):
        raise ValueError("4:2:2 frames have even width and height")
    if v not in (PIX_UYVY422, PIX_YUYV422, PIX_YUV422P, PIX_NV16):
        raise ValueError("not a 4:2:2 layout")
    rows, cols = frame_shape(v, w, h)
    if f.ndim != 2 or f.dtype != np.uint8 or f.shape[0] != rows or f.shape[1] < cols:
        raise ValueError("expected a uint8 frame of %d rows and at least %d columns" % (rows, cols))
    f = f[:, :cols]
    if v == PIX_UYVY422:
        return f[:, 1::2], f[:, 0::4], f[:, 2::4]
    if v == PIX_YUYV422:
        return f[:, 0::2], f[:, 1::4], f[:, 3::4]
    if v == PIX_YUV422P:
        return f[:h], f[h:, :w // 2], f[h:, w // 2:]
    return f[:h], f[h:, 0::2], f[h:, 1::2]


def yuv420p_from_yuv422(fmt, frame, w, h):
    """The "Y over [U|V]" frame of a frame in the 4:2:2 layout `fmt` by the library's input rule: chroma row r is
    (c[2r] + c[2r + 1] + 1) >> 1 per byte of chroma rows 2r and 2r + 1, for U and V; luma is copied."""
    y, u, v = yuv422_planes(fmt, frame, w, h)
    w, h = int(w), int(h)
    out = np.empty((h * 3 // 2, w), np.uint8)
    out[:h] = y
    for plane, x0 in ((u, 0), (v, w // 2)):
        c = plane.astype(np.uint16)
        out[h:, x0:x0 + w // 2] = ((c[0::2] + c[1::2] + 1) >> 1).astype(np.uint8)
    return out


def _yuv10_layout(fmt):
    v = _pix_value(fmt)
    if v not in _PIX_10BIT:
        raise ValueError("not a 10-bit layout")
    return v, v in (PIX_P210, PIX_YUV422P10), v in (PIX_YUV420P10, PIX_YUV422P10)


def yuv10_from_yuv420p(fmt, frame, w, h):
    """The frame in the 10-bit layout `fmt` ("p010", "yuv420p10", "p210", "yuv422p10" or the PIX_* value) of an 8-bit
    "Y over [U|V]" frame by the library's output rule: v10 = v8 << 2 (the word v8 << 8 for "p010" / "p210", v8 << 2
    for the planar two), the 4:2:2 layouts with chroma row r on rows 2r and 2r + 1.  A uint16 array of
    frame_shape(fmt, w, h)[0] rows and w words; .view(numpy.uint8) is the frame in bytes."""
    v, c422, planar = _yuv10_layout(fmt)
    f, w, h = _chroma_frame(frame, w, h)
    u, vv = f[h:, :w // 2], f[h:, w // 2:w]
    if c422:
        u, vv = np.repeat(u, 2, axis=0), np.repeat(vv, 2, axis=0)
    out = np.empty((frame_shape(v, w, h)[0], w), np.uint16)
    out[:h] = f[:h, :w]
    if planar:
        out[h:, :w // 2], out[h:, w // 2:] = u, vv
    else:
        out[h:, 0::2], out[h:, 1::2] = u, vv
    return out << (2 if planar else 8)


def yuv420p_from_yuv10(fmt, frame, w, h):
    """The 8-bit "Y over [U|V]" frame of a frame in the 10-bit layout `fmt` (uint16 words, or uint8 with two columns
    per word; columns past a row's width are dropped) by the library's input rule: v8 = min(255, (v10 + 2) >> 2) per
    sample, v10 bits 15..6 of a "p010" / "p210" word and bits 9..0 of a planar one; the 4:2:2 layouts then take
    (c8[2r] + c8[2r + 1] + 1) >> 1 of the narrowed chroma rows 2r and 2r + 1."""
    v, c422, planar = _yuv10_layout(fmt)
    f = np.asarray(frame)
    w, h = int(w), int(h)
    if w <= 0 or h <= 0 or (w & 1) or (h & 1):
        raise ValueError("10-bit frames have even width and height")
    if f.ndim == 2 and f.dtype == np.uint8 and f.shape[1] % 2 == 0:
        f = np.ascontiguousarray(f).view(np.uint16)
    rows = frame_shape(v, w, h)[0]
    if f.ndim != 2 or f.dtype != np.uint16 or f.shape[0] != rows or f.shape[1] < w:
        raise ValueError("expected a frame of %d rows and at least %d 16-bit words a row" % (rows, w))
    v10 = (f[:, :w] & 0x3FF if planar else f[:, :w] >> 6).astype(np.int32)
    v8 = np.minimum(255, (v10 + 2) >> 2)
    c = v8[h:]
    u, vv = (c[:, :w // 2], c[:, w // 2:]) if planar else (c[:, 0::2], c[:, 1::2])
    if c422:
        u, vv = (u[0::2] + u[1::2] + 1) >> 1, (vv[0::2] + vv[1::2] + 1) >> 1
    out = np.empty((h * 3 // 2, w), np.uint8)
    out[:h], out[h:, :w // 2], out[h:, w // 2:] = v8[:h], u, vv
    return out


class Mapper:
    """vr::Mapper on one device: stitch(inputs YUV420P, output YUV420P) with optional gain.

    A template with K overlays (mt.num_overlays) takes N + K in_sizes and N + K frames per stitch: the tail
    frames are the overlays' live frames, in overlay order, each of its own (even) size.  They are warped
    like the inputs (vignette included), never gained or blended, and copied onto the blended result where
    their mask is set, a later overlay over an earlier one, before the scaled output and the preview are
    taken.  gains() and the `gains` argument keep one entry per input (N)."""

    def __init__(self, mt, in_sizes, blend=0, enable_gain=True, device=0, scale_output=(0, 0), remap="remap"):
        """remap: "remap" (cv::remap's fixed point, the default) or "texture" (the reference's CUDA
        fastRemap texture sampling, OCTVR_REMAP_TEXTURE)."""
        n = len(in_sizes)
        w = (C.c_int * n)(*[s[0] for s in in_sizes])
        h = (C.c_int * n)(*[s[1] for s in in_sizes])
        scale_output = tuple(scale_output) if scale_output else (0, 0)  # None / () = unscaled
        if remap not in ("remap", "texture"):
            raise ValueError("remap must be 'remap' or 'texture'")
        hd = _VP()
        if remap == "texture":
            _check(_lib.octvr_mapper_create_ex(mt._h, device, n, w, h, blend, int(enable_gain), scale_output[0],
                                               scale_output[1], REMAP_TEXTURE, C.byref(hd)))
        else:
            _check(_lib.octvr_mapper_create(mt._h, device, n, w, h, blend, int(enable_gain), scale_output[0],
                                            scale_output[1], C.byref(hd)))
        self._h = hd
        self._mt = mt  # prepare_preview builds its list from the template's maps
        self.n = n  # frames per stitch: inputs, then overlays
        self.n_gains = n - mt.num_overlays
        self.device = device
        # output frame size: scale_output, or the template's out_size (mapper.cpp:69)
        self.out_size = tuple(scale_output) if scale_output[0] else mt.out_size

    @staticmethod
    def frame_refs(inputs):
        """FrameRefs of a list of input tensors, accepted by stitch() in place of the list."""
        return FrameRefs(inputs)

    def stitch(self, inputs, output, gains=None, stream=None, preview=None):
        """inputs: list of uint8 cuda tensors (1.5H x W "Y over [U|V]") or their FrameRefs; output likewise.
        preview: an optional (h, w, 3) uint8 cuda tensor receiving Mapper::stitch's preview_output (the RGB
        result resized, mapper.cpp:308-312; of the size prepare_preview prepared: gathered from the source
        frames, no result frame).  stream: a torch stream or a raw ctypes stream handle."""
        if isinstance(inputs, FrameRefs):
            n, ptrs, pitches = inputs.n, inputs.ptrs, inputs.pitches
        else:
            n = len(inputs)
            ptrs = (_VP * n)(*[t.data_ptr() for t in inputs])
            pitches = (C.c_size_t * n)(*[t.stride(0) for t in inputs])
        if n != self.n:
            raise ValueError("stitch takes %d frames (every input, then every overlay), got %d" % (self.n, n))
        g = None
        ng = 0
        if gains is not None:
            g = (C.c_double * len(gains))(*gains)
            ng = len(gains)
        if preview is None:
            _check(_lib.octvr_mapper_stitch_yuv420p(self._h, ptrs, pitches, C.c_void_p(output.data_ptr()),
                                                    output.stride(0), g, ng, _stream_ptr(stream)))
        else:
            assert preview.dim() == 3 and preview.shape[2] == 3 and preview.stride(1) == 3 and preview.stride(2) == 1
            _check(_lib.octvr_mapper_stitch_preview(self._h, ptrs, pitches, C.c_void_p(output.data_ptr()),
                                                    output.stride(0), C.c_void_p(preview.data_ptr()),
                                                    preview.shape[1], preview.shape[0], preview.stride(0), g, ng,
                                                    _stream_ptr(stream)))

    def prepare_preview(self, w, h):
        """Prepares a w x h preview that needs no result frame (octvr_mapper_prepare_preview): afterwards
        stitch(preview=...) with a tensor of that size runs the stitch without a preview plus one gather kernel,
        with any number of frames in flight, and gives the same bytes; other sizes stay on the result-frame
        path.  Blend 0 and unscaled output only (OctvrError E_UNSUPPORTED otherwise); a second call replaces
        the size, (0, 0) drops it.  Synchronizes."""
        _check(_lib.octvr_mapper_prepare_preview(self._h, self._mt._h, int(w), int(h)))

    def stitch_tensor(self, inputs, tensor, output=None, gains=None, stream=None, order="rgb", scale=None, bias=None):
        """The RGB result as a planar tensor for a model (octvr_mapper_stitch_tensor).  tensor: a (3, h, w) cuda
        tensor of uint8, float16 or float32 with stride(2) == 1; stride(0) and stride(1) are the plane and row
        strides, so a view into a batch tensor works.  Plane p holds colour p of order ("rgb" or "bgr") of the
        bytes P a (h, w, 3) preview of the same stitch would hold: P for uint8, P * scale[c] + bias[c] in float32
        (a multiply, then an add; rounded to nearest even for float16) otherwise.  scale, bias: a scalar or three
        values for R, G, B (defaults 1 and 0; ignored for uint8).  output: the YUV frame as stitch() writes it, or
        None for no YUV frame.  A tensor of the size prepare_preview prepared is gathered from the source frames
        (any number of frames in flight; with output=None no composite is launched); any other size is resized
        from the result frame and needs one frame in flight."""
        dtypes = {torch.uint8: TENSOR_U8, torch.float16: TENSOR_F16, torch.float32: TENSOR_F32}
        if not isinstance(tensor, torch.Tensor) or tensor.dim() != 3 or tensor.shape[0] != 3:
            raise ValueError("tensor must be a torch tensor of shape (3, h, w)")
        if tensor.dtype not in dtypes:
            raise ValueError("tensor dtype must be uint8, float16 or float32")
        if tensor.device.type != "cuda" or tensor.device.index != self.device:
            raise ValueError("tensor must be on the mapper's device cuda:%d" % self.device)
        if tensor.shape[1] < 1 or tensor.shape[2] < 1 or (tensor.shape[2] > 1 and tensor.stride(2) != 1):
            raise ValueError("tensor needs stride(2) == 1 (planes of contiguous rows)")
        if order not in ("rgb", "bgr"):
            raise ValueError("order must be 'rgb' or 'bgr'")

        def three(v, default, name):
            if v is None:
                v = default
            vals = [float(x) for x in np.asarray(v, dtype=np.float32).reshape(-1)]
            if len(vals) == 1:
                vals = vals * 3
            if len(vals) != 3:
                raise ValueError("%s takes a scalar or three values (R, G, B)" % name)
            return (C.c_float * 3)(*vals)

        t = TensorOut(tensor.data_ptr(), tensor.shape[2], tensor.shape[1], dtypes[tensor.dtype], int(order == "bgr"),
                      max(tensor.stride(1), 0), max(tensor.stride(0), 0), three(scale, 1.0, "scale"),
                      three(bias, 0.0, "bias"))
        if isinstance(inputs, FrameRefs):
            n, ptrs, pitches = inputs.n, inputs.ptrs, inputs.pitches
        else:
            n = len(inputs)
            ptrs = (_VP * n)(*[x.data_ptr() for x in inputs])
            pitches = (C.c_size_t * n)(*[x.stride(0) for x in inputs])
        if n != self.n:
            raise ValueError("stitch takes %d frames (every input, then every overlay), got %d" % (self.n, n))
        g = None
        ng = 0
        if gains is not None:
            g = (C.c_double * len(gains))(*gains)
            ng = len(gains)
        out_ptr = C.c_void_p(output.data_ptr()) if output is not None else None
        _check(_lib.octvr_mapper_stitch_tensor(self._h, ptrs, pitches, out_ptr, output.stride(0) if output is not None else 0,
                                               C.byref(t), g, ng, _stream_ptr(stream)))

    @staticmethod
    def batch_refs(frame_sets, outputs):
        """BatchRefs of several frame sets (lists of input tensors or FrameRefs) and their outputs, accepted
        by stitch_batch() in place of the lists."""
        return BatchRefs(frame_sets, outputs)

    def stitch_batch(self, frame_sets, outputs=None, gains=None, stream=None):
        """len(frame_sets) (1, 2 or 4) frames in one call (octvr_mapper_stitch_batch): each frame's gains
        estimated (or gains: one list per frame), one composite launch for all; outputs: one tensor per
        frame (same pitch).  frame_sets may be a BatchRefs (outputs then None)."""
        b = frame_sets if isinstance(frame_sets, BatchRefs) else BatchRefs(frame_sets, outputs)
        g = None
        if gains is not None:
            flat = [float(v) for gl in gains for v in gl]
            g = (C.c_double * len(flat))(*flat)
        _check(_lib.octvr_mapper_stitch_batch(self._h, b.nf, b.ptrs, b.pitches, b.outs, b.out_pitch, g,
                                              _stream_ptr(stream)))

    def gains(self):
        g = (C.c_double * self.n_gains)()
        _check(_lib.octvr_mapper_gains(self._h, g, self.n_gains))
        return list(g)

    def set_frames_in_flight(self, k):
        """k slots of per-frame device state: stitches issued on different streams overlap
        (octvr_mapper_set_frames_in_flight).  No scaled output, and no overlays on a multi-band / feather
        mapper (one result frame); multi-band / feather mappers get per-slot pyramids."""
        _check(_lib.octvr_mapper_set_frames_in_flight(self._h, int(k)))

    def set_pixel_formats(self, in_format="yuv420p", out_format="yuv420p"):
        """Layouts of the input frames (all alike) and of the output of every later stitch / stitch_batch:
        "yuv420p" ("Y over [U|V]", the default), "nv12" (chroma rows of U,V byte pairs), "uyvy422" (packed
        4:2:2, h rows of 2w bytes, converted to and from 4:2:0 frames of the mapper's own by one launch each),
        "yuyv422" (packed, Y0 U0 Y1 V0), "yuv422p" or "nv16" (2h rows of w bytes: Y over h chroma rows, [U|V]
        halves or U,V pairs; frame_shape gives each layout's shape), the 10-bit "p010", "yuv420p10", "p210" or
        "yuv422p10" (16-bit little-endian words, rows of 2w bytes, base and pitch multiples of 2; narrowed to and
        widened from the mapper's 8-bit frames by v8 = min(255, (v10 + 2) >> 2) and v10 = v8 << 2: the stitch stays
        the 8-bit one; uint8 tensors of frame_shape, e.g. a uint16 tensor's .view(torch.uint8)), "v210" (10-bit 4:2:2
        in 32-bit words, h rows of v210_row_bytes(w) bytes, base and pitch multiples of 4; P210's two rules), or the
        OCTVR_PIX_* values (octvr_mapper_set_pixel_formats).  Synchronizes."""
        _check(_lib.octvr_mapper_set_pixel_formats(self._h, _pix_value(in_format), _pix_value(out_format)))

    @property
    def pixel_formats(self):
        """(input layout, output layout) as "yuv420p" / "nv12" / "uyvy422" / "yuyv422" / "yuv422p" / "nv16" / "p010" /
        "yuv420p10" / "p210" / "yuv422p10" / "v210"."""
        a, b = C.c_int(), C.c_int()
        _check(_lib.octvr_mapper_pixel_formats(self._h, C.byref(a), C.byref(b)))
        return _PIX_BY_VALUE[a.value], _PIX_BY_VALUE[b.value]

    def traffic_bytes(self):
        b = C.c_double()
        _check(_lib.octvr_mapper_traffic(self._h, C.byref(b)))
        return b.value

    def traffic_parts(self):
        """(lut bytes read once per launch, bytes per frame) of the composite (octvr_mapper_traffic_parts)."""
        a, b = C.c_double(), C.c_double()
        _check(_lib.octvr_mapper_traffic_parts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def info(self):
        buf = C.create_string_buffer(8192)
        _check(_lib.octvr_mapper_info(self._h, buf, 8192))
        return _json.loads(buf.value.decode())

    def set_timing(self, enable=True):
        _check(_lib.octvr_mapper_set_timing(self._h, int(enable)))

    def kernel_time(self):
        """(total device ms, launches) of the composite kernel since the last call (synchronizes)."""
        t, k = C.c_double(), C.c_int()
        _check(_lib.octvr_mapper_kernel_time(self._h, C.byref(t), C.byref(k)))
        return t.value, k.value

    def kernel_busy(self):
        """(summed start-to-end ms, union ms, launches) of the logged launches (synchronizes)."""
        sp, bu, k = C.c_double(), C.c_double(), C.c_int()
        _check(_lib.octvr_mapper_kernel_busy(self._h, C.byref(sp), C.byref(bu), C.byref(k)))
        return sp.value, bu.value, k.value

    def kernel_intervals(self, cap=4096):
        """[(start ms, end ms)] of the logged launches relative to the first one's start, in issue order
        (synchronizes; clears the log as kernel_busy does)."""
        st, en, k = (C.c_double * cap)(), (C.c_double * cap)(), C.c_int()
        _check(_lib.octvr_mapper_kernel_intervals(self._h, st, en, cap, C.byref(k)))
        return [(st[i], en[i]) for i in range(min(k.value, cap))]

    def close(self):
        if self._h and self._h.value:
            _lib.octvr_mapper_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FastMapper:
    """vr::FastMapper (modules/octvr/src/mapper_fast.cpp): feather-weighted NV12 stitch of a full-frame rig."""

    def __init__(self, mt, in_sizes, device=0):
        n = len(in_sizes)
        w = (C.c_int * n)(*[s[0] for s in in_sizes])
        h = (C.c_int * n)(*[s[1] for s in in_sizes])
        hd = _VP()
        _check(_lib.octvr_fastmapper_create(mt._h, device, n, w, h, C.byref(hd)))
        self._h = hd
        self.n = n
        self.out_size = mt.out_size

    def traffic_bytes(self):
        """Algorithmic bytes of one stitch_nv12 (octvr_fastmapper_traffic)."""
        b = C.c_double()
        _check(_lib.octvr_fastmapper_traffic(self._h, C.byref(b)))
        return b.value

    def stitch_nv12(self, inputs, output, stream=None):
        """inputs: uint8 cuda tensors (1.5H x W NV12) or their FrameRefs; output: 1.5H x W (chroma rows V,U)."""
        if isinstance(inputs, FrameRefs):
            n, ptrs, pitches = inputs.n, inputs.ptrs, inputs.pitches
        else:
            n = len(inputs)
            ptrs = (_VP * n)(*[t.data_ptr() for t in inputs])
            pitches = (C.c_size_t * n)(*[t.stride(0) for t in inputs])
        _check(_lib.octvr_fastmapper_stitch_nv12(self._h, ptrs, pitches, C.c_void_p(output.data_ptr()), output.stride(0),
                                                 _stream_ptr(stream)))

    def traffic_parts(self):
        """(entry bytes read once per launch, bytes per frame) of one stitch (octvr_fastmapper_traffic_parts)."""
        a, b = C.c_double(), C.c_double()
        _check(_lib.octvr_fastmapper_traffic_parts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def stitch_nv12_batch(self, frame_sets, outputs=None, stream=None):
        """len(frame_sets) (1, 2 or 4) frames in one launch per plane (octvr_fastmapper_stitch_nv12_batch); outputs:
        one tensor per frame (same pitch).  frame_sets may be a BatchRefs (outputs then None)."""
        b = frame_sets if isinstance(frame_sets, BatchRefs) else BatchRefs(frame_sets, outputs)
        _check(_lib.octvr_fastmapper_stitch_nv12_batch(self._h, b.nf, b.ptrs, b.pitches, b.outs, b.out_pitch,
                                                       _stream_ptr(stream)))

    def close(self):
        if self._h and self._h.value:
            _lib.octvr_fastmapper_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AsyncMultiMapper:
    """vr::AsyncMultiMapper (modules/octvr/src/async.cpp): host YUV420P planes in, host planes out, through
    a 3-deep pinned-buffer pipeline (copy-in, H2D, stitch, D2H, copy-out overlap across frames).  Either side
    may be NV12 instead (set_pixel_formats): its plane sets are then (Y, UV) two-tuples.  Frames that already
    live on the device go through push_device() instead of push(): cuda tensors in, one merged cuda tensor
    out, no host copy; both kinds may be mixed on one pipeline.

    templates: list of MapperTemplate over the same len(in_sizes) frames: each template's inputs plus its
    overlays number len(in_sizes) (the split may differ per template; the overlays' frames are the tail, as
    for Mapper); output_regions: list of (x, y, w, h)
    fractions of out_size; gain_modes[i]: -1 no gain, i estimate, j < i reuse mapper j's gains (template j
    then has as many inputs as template i).
    preview_size (w, h): AsyncMultiMapper::New's preview — each mapper also writes its region of one RGB
    preview image every frame (async.cpp:73-110); read the latest with preview(), or receive every one
    through set_preview_sink()."""

    def __init__(self, templates, in_sizes, out_size, blend_modes, gain_modes, output_regions, device=0, remap="remap",
                 preview_size=(0, 0)):
        if remap not in ("remap", "texture"):
            raise ValueError("remap must be 'remap' or 'texture'")
        self._h = C.c_void_p(0)
        k, n = len(templates), len(in_sizes)
        rigs = (_VP * k)(*[t._h.value for t in templates])
        w = (C.c_int * n)(*[s[0] for s in in_sizes])
        h = (C.c_int * n)(*[s[1] for s in in_sizes])
        bm = (C.c_int * k)(*blend_modes)
        gm = (C.c_int * k)(*gain_modes)
        rg = (C.c_double * (4 * k))(*[float(v) for r in output_regions for v in r])
        hd = _VP()
        pw, ph = (int(v) for v in preview_size)
        if pw or ph:
            _check(_lib.octvr_async_create_preview(rigs, k, device, n, w, h, out_size[0], out_size[1], bm, gm, rg,
                                                   REMAP_TEXTURE if remap == "texture" else 0, pw, ph, C.byref(hd)))
        elif remap == "texture":
            _check(_lib.octvr_async_create_ex(rigs, k, device, n, w, h, out_size[0], out_size[1], bm, gm, rg,
                                              REMAP_TEXTURE, C.byref(hd)))
        else:
            _check(_lib.octvr_async_create(rigs, k, device, n, w, h, out_size[0], out_size[1], bm, gm, rg, C.byref(hd)))
        self._h = hd
        self.preview_size = (pw, ph) if pw * ph > 0 else (0, 0)
        self._sink = None
        self._registered = []
        self._templates = list(templates)  # the mappers copy what they need; kept for symmetry with the reference
        self.n = n
        self.in_sizes = [(int(s[0]), int(s[1])) for s in in_sizes]
        self.out_size = tuple(out_size)
        self._inflight = []

    def push(self, inputs, output):
        """inputs: list of (Y, U, V) uint8 numpy planes per camera; output: (Y, U, V) planes of the merged
        frame; a side that is NV12 takes (Y, UV) — UV the interleaved plane of W bytes x H/2 rows — with an
        optional third entry that is ignored.  4:2:2 inputs (set_pixel_formats): "uyvy422" / "yuyv422" one packed
        plane (h rows of 2w bytes), as a one-tuple or the array itself; "yuv422p" (Y, U, V) with U and V of h rows
        of w/2 bytes; "nv16" (Y, UV) with UV of h rows of w bytes.  10-bit inputs, planes of 16-bit words given as
        uint16 arrays or as their bytes (uint8, even pitches): "p010" / "p210" (Y, UV) with Y of h rows of w words
        and UV of h/2 or h rows of w words (U,V pairs); "yuv420p10" / "yuv422p10" (Y, U, V) with U and V of h/2 or
        h rows of w/2 words.  The arrays are kept alive until the matching pop()."""
        fix = lambda p: p if p is None or p.strides[1] == p.itemsize else np.ascontiguousarray(p)
        inputs = [(tri,) if isinstance(tri, np.ndarray) else tuple(tri) for tri in inputs]  # a packed UYVY plane
        ip, ipt, planes = _plane_args([tuple(fix(p) for p in tri) for tri in inputs])
        op, opt, _ = _plane_args([self._output_planes(output)])
        _check(_lib.octvr_async_push(self._h, ip, ipt, op, opt))
        self._inflight.append((planes, output))

    def _output_planes(self, output):
        """The output plane set as a tuple; with a converted output format (set_output_format) its planes are
        checked against plane_shapes: uint8 arrays, or for the 16-bit layouts uint16 arrays or their bytes."""
        fmt = self.pixel_formats[1]
        if _PIX_BY_NAME[fmt] in (PIX_YUV420P, PIX_NV12):
            return output
        planes = (output,) if isinstance(output, np.ndarray) else tuple(output)
        want = plane_shapes(fmt, self.out_size[0], self.out_size[1])
        if len(planes) < len(want):
            raise ValueError("output: %s takes %d planes, got %d" % (fmt, len(want), len(planes)))
        for k, (rows, nbytes) in enumerate(want):
            p = planes[k]
            if not (isinstance(p, np.ndarray) and p.ndim == 2 and p.dtype in (np.uint8, np.uint16) and
                    p.strides[1] == p.itemsize and p.shape[0] == rows and p.shape[1] * p.itemsize == nbytes):
                raise ValueError("output plane %d: expected %d rows of %d bytes (%s) with unit column stride"
                                 % (k, rows, nbytes, fmt))
        return planes[:len(want)]

    @staticmethod
    def _device_frame(t, w, h, what, fmt="yuv420p"):
        """t as a device frame of a w x h picture: a 2-D cuda uint8 tensor of 3h/2 rows and w columns (h rows and
        2w columns for "uyvy422"; frame_shape(fmt, w, h) in general) with unit column stride (a view of a larger
        tensor is fine: its row stride is the pitch)."""
        shape = frame_shape(fmt, w, h)
        if not (hasattr(t, "is_cuda") and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and
                tuple(t.shape) == shape and t.stride(1) == 1):
            raise ValueError("%s: expected a cuda uint8 tensor of shape (%d, %d) with unit column stride"
                             % ((what,) + shape))
        return t

    def push_device(self, inputs, output, ready=None):
        """push() for frames that live on the device (octvr_async_push_device): inputs, one 2-D cuda uint8
        tensor per input and then per overlay (3h/2 rows x w columns, "Y over [U|V]" or NV12 as the input
        format says), are read in place; output, one such tensor of the merged frame (3H/2 x W), is written on
        the device, bytes outside the regions and past the width untouched.  A tensor's row stride is its
        pitch, so views of larger tensors work.  ready: a recorded torch.cuda.Event the stitch waits for before
        it reads the inputs; None: the inputs are complete (synchronize the stream that wrote them first).
        The tensors are kept alive until the matching pop(), which returns `output` once the merged frame is
        complete on the device.  With a 10-bit input format the inputs are uint8 tensors of frame_shape(fmt, w, h)
        (rows of 2w bytes; a uint16 tensor's .view(torch.uint8)) at even addresses and pitches."""
        if len(inputs) != self.n:
            raise ValueError("push_device takes %d frames (every input, then every overlay), got %d"
                             % (self.n, len(inputs)))
        fmt = self.pixel_formats[0]
        ins = [self._device_frame(t, w, h, "input %d" % i, fmt) for i, (t, (w, h)) in enumerate(zip(inputs, self.in_sizes))]
        out = self._device_frame(output, self.out_size[0], self.out_size[1], "output", self.pixel_formats[1])
        ptrs = (_VP * self.n)(*[t.data_ptr() for t in ins])
        pitches = (C.c_size_t * self.n)(*[t.stride(0) for t in ins])
        ev = None
        if ready is not None:
            ev = C.c_void_p(ready.cuda_event)
            if not ev.value:
                raise ValueError("ready: the event has not been recorded")
        _check(_lib.octvr_async_push_device(self._h, ptrs, pitches, C.c_void_p(out.data_ptr()), out.stride(0), ev))
        self._inflight.append(((ins, ready), output))

    def pop(self):
        """Blocks until the oldest pushed frame is written; returns its output planes (push_device: its
        output tensor)."""
        rc = _lib.octvr_async_pop(self._h)
        output = self._inflight.pop(0)[1] if self._inflight else None
        _check(rc)
        return output

    def pending(self):
        n = C.c_int()
        _check(_lib.octvr_async_pending(self._h, C.byref(n)))
        return n.value

    def register_output(self, output):
        """Page-lock an output (Y, U, V) plane set — (Y, UV) with an NV12 output — the caller will push again
        (octvr_async_register_output): its frames are then downloaded straight into it.  Planes that are
        views of one array (a contiguous NV12 frame's a[:H] and a[H:]) are locked as one range.  The arrays are
        kept alive until close()."""
        output = self._output_planes(output)
        op, opt, _ = _plane_args([output])
        _check(_lib.octvr_async_register_output(self._h, op, opt))
        self._registered.append(tuple(output))

    def unregister_output(self, output):
        output = (output,) if isinstance(output, np.ndarray) else output
        op, _, _ = _plane_args([output])
        _check(_lib.octvr_async_unregister_output(self._h, op))
        self._registered = [r for r in self._registered
                            if not (len(r) == len(output) and all(a is b for a, b in zip(r, output)))]

    def set_pixel_formats(self, in_format="yuv420p", out_format="yuv420p"):
        """Layouts of the host planes of every later push, "yuv420p" (the default) or "nv12", or the
        OCTVR_PIX_* values (octvr_async_set_pixel_formats): no frame may be pending, and the output format
        cannot change while output plane sets are registered.  The input format may also be "uyvy422": push then
        takes one packed plane (h rows of 2w bytes) per camera, as a one-tuple or the array itself, and
        push_device one packed cuda tensor per camera; as the output format it is E_UNSUPPORTED here (set_output_format
        sets the converted layouts as the output format).  "yuyv422",
        "yuv422p" and "nv16" likewise: input only, planes as push() describes, push_device one cuda tensor of
        frame_shape(fmt, w, h) per camera.  So are the 10-bit "p010", "yuv420p10", "p210" and "yuv422p10": one
        narrowing conversion per frame serves all mappers, which read the pipeline's 8-bit NV12 frames.  "v210" too is
        an input format (one plane or cuda tensor of h rows of v210_row_bytes(w) bytes per camera, base and pitch
        multiples of 4); as the output format it is E_UNSUPPORTED here and from set_output_format: v210 out of the
        pipeline is not built."""
        _check(_lib.octvr_async_set_pixel_formats(self._h, _pix_value(in_format), _pix_value(out_format)))

    def set_output_format(self, out_format):
        """The layout of the merged frame, any of the ten names or OCTVR_PIX_* values
        (octvr_async_set_output_format).  "yuv420p" and "nv12" are set_pixel_formats(current input format, it).  A
        converted layout keeps the input format, puts the mappers on NV12 output and has one kernel per frame merge
        and convert their region frames: push and register_output then take the layout's planes (plane_shapes: one
        packed plane, as a one-tuple or the array itself; (Y, UV); or (Y, U, V); uint8 arrays or, for the 16-bit
        layouts, uint16 arrays or their bytes), push_device an output tensor of frame_shape(fmt, W, H) bytes.  Every
        region must start at even x and y with its chroma rectangle at their halves (E_INVALID otherwise, as with
        frames pending or output planes registered in another format).  set_pixel_formats(in, "yuv420p" or "nv12")
        leaves converted output."""
        _check(_lib.octvr_async_set_output_format(self._h, _pix_value(out_format)))

    @property
    def pixel_formats(self):
        a, b = C.c_int(), C.c_int()
        _check(_lib.octvr_async_pixel_formats(self._h, C.byref(a), C.byref(b)))
        return _PIX_BY_VALUE[a.value], _PIX_BY_VALUE[b.value]

    def preview(self):
        """(rgb, header): the latest published preview as an (h, w, 3) uint8 array and its PreviewDataHeader
        (width 0 and rgb None before the first frame completes)."""
        pw, ph = self.preview_size
        rgb = np.zeros((max(ph, 1), max(pw, 1), 3), np.uint8)
        hdr = PreviewDataHeader()
        _check(_lib.octvr_async_pop_preview(self._h, rgb.ctypes.data, rgb.strides[0], C.byref(hdr)))
        return (rgb if hdr.width else None), hdr

    def set_preview_sink(self, fn):
        """fn(rgb, header) on the pipeline's copy-out thread for every frame's preview (rgb: a copy); None
        removes it."""
        if fn is None:
            _check(_lib.octvr_async_set_preview_sink(self._h, PREVIEW_SINK(), None))
            self._sink = None
            return
        pw, ph = self.preview_size

        def _cb(user, p, pitch, hdr):
            a = np.ctypeslib.as_array(p, shape=(ph * pitch,)).reshape(ph, pitch)[:, :pw * 3].reshape(ph, pw, 3).copy()
            h = hdr.contents
            fn(a, PreviewDataHeader(h.width, h.height, h.step, h.fps))

        cb = PREVIEW_SINK(_cb)
        _check(_lib.octvr_async_set_preview_sink(self._h, cb, None))
        self._sink = cb  # keep the ctypes thunk alive

    def info(self):
        """Build-time facts of the pipeline (octvr_async_info): packed_bytes uploaded per frame, runs, ..."""
        buf = C.create_string_buffer(1024)
        _check(_lib.octvr_async_info(self._h, buf, len(buf)))
        import json as _json
        return _json.loads(buf.value.decode())

    def close(self):
        if self._h and self._h.value:
            _lib.octvr_async_destroy(self._h)
            self._h = C.c_void_p(0)
            self._inflight = []
            self._registered = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_lib.octvr_selftest_sat_u8.argtypes = [_VP, _VP, C.c_int, C.c_int, _VP]


def selftest_sat_u8(values, method, stream=None):
    """Device float -> u8 saturating conversion (kernel self-test)."""
    x = values if isinstance(values, torch.Tensor) else torch.tensor(values, dtype=torch.float32)
    x = x.to(device="cuda", dtype=torch.float32).contiguous()
    out = torch.empty(x.numel(), dtype=torch.uint8, device=x.device)
    _check(_lib.octvr_selftest_sat_u8(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), x.numel(), method,
                                      _stream_ptr(stream)))
    return out


def remap_u8(src, map1, map2, scale_x, scale_y, out=None, stream=None):
    """cv::remap INTER_LINEAR on cuda uint8 tensors (H x W [x cn]); maps are cuda float32 (mh x mw)."""
    cn = 1 if src.dim() == 2 else src.shape[2]
    mh, mw = map1.shape
    if out is None:
        out = torch.empty((mh, mw) if cn == 1 else (mh, mw, cn), dtype=torch.uint8, device=src.device)
    _check(_lib.octvr_remap_u8(C.c_void_p(src.data_ptr()), src.shape[1], src.shape[0], src.stride(0), cn,
                               C.c_void_p(map1.data_ptr()), C.c_void_p(map2.data_ptr()), mw, mh, map1.stride(0),
                               scale_x, scale_y, C.c_void_p(out.data_ptr()), out.stride(0), _stream_ptr(stream)))
    return out


def fill_poly(img, pts, color):
    """cv::fillPoly(img, {pts}, color) on a 2-D uint8 numpy array, in place (octvr_fill_poly_u8)."""
    import numpy as np
    assert img.dtype == np.uint8 and img.ndim == 2 and img.flags.c_contiguous
    flat = np.ascontiguousarray(np.asarray(pts, np.int32).reshape(-1))
    _check(_lib.octvr_fill_poly_u8(img.ctypes.data, img.shape[1], img.shape[0],
                                   flat.ctypes.data_as(C.POINTER(C.c_int)), len(flat) // 2, color))
    return img


def png_decode_rgb(data):
    """cv::imdecode(png, IMREAD_COLOR) with the channels in R,G,B order (octvr_png_decode_rgb)."""
    import numpy as np
    w, h = C.c_int(), C.c_int()
    _check(_lib.octvr_png_decode_rgb(data, len(data), None, 0, C.byref(w), C.byref(h)))
    out = np.empty((h.value, w.value, 3), np.uint8)
    _check(_lib.octvr_png_decode_rgb(data, len(data), out.ctypes.data, out.nbytes, C.byref(w), C.byref(h)))
    return out
