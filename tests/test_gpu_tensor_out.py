"""Mapper.stitch_tensor (octvr_mapper_stitch_tensor, csrc/tensor_out.hip): the RGB result as a planar u8 / f16 /
f32 tensor, resized from the result frame or gathered through the prepared tap list.

The reference of every case: P = the oracle's preview of the same stitch (oracle_py.stitch_frame(...,
preview=(w, h)); tests/overlay_ref.py for the overlay rig), and this file's own numpy on it,
P[..., c].astype(float32) * float32(scale) + float32(bias), then .astype(float16) for f16.  Compared as integer
views, tolerance 0.  rigA's golden arrays; noise chroma over smooth luma, so that P takes every byte value."""
import copy
import ctypes as C
import functools
import json

import numpy as np
import pytest

import camera_rigs as R
import oracle_py as O
import overlay_ref as OR

pytestmark = pytest.mark.gpu

SMALL = (301, 151)   # odd, no upscale, weights from unclamped coordinates
WIDE16 = (257, 129)  # 16 k + 1 pixels wide
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
NP_OF = {"u8": np.uint8, "f16": np.float16, "f32": np.float32}
INT_OF = {"u8": np.uint8, "f16": np.uint16, "f32": np.uint32}


@functools.lru_cache(maxsize=None)
def _rig():
    rig, z = O.load_rig("rigA")
    n = len(z["rois"])
    W, H = (int(v) for v in z["out_size"])
    return {"rig": rig, "W": W, "H": H, "n": n, "rois": z["rois"].tolist(),
            "sizes": [(rig["inputs"][i]["options"]["width"], rig["inputs"][i]["options"]["height"]) for i in range(n)],
            "map1": [z[f"map1_{i}"] for i in range(n)], "map2": [z[f"map2_{i}"] for i in range(n)],
            "masks": [z[f"mask_{i}"] for i in range(n)], "seams": [z[f"seam_{i}"] for i in range(n)]}


def _template(ox, t):
    return ox.MapperTemplate.from_arrays(t["W"], t["H"], t["rois"], t["map1"], t["map2"], t["masks"], t["seams"])


def _noise_frame(w, h, seed):
    """Smooth luma, noise chroma (as tests/test_gpu_async_yuv422.py makes its pictures), YUV420P."""
    from octvr_amd import synthetic
    f = synthetic.smooth_yuv_frame(w, h, seed).copy()
    f[h:] = np.random.RandomState(seed).randint(0, 256, (h // 2, w), dtype=np.int64).astype(np.uint8)
    return f


@functools.lru_cache(maxsize=None)
def _frames(seed):
    fr = tuple(_noise_frame(w, h, seed + i) for i, (w, h) in enumerate(_rig()["sizes"]))
    for f in fr:
        f.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def _want(seed, preview, blend=0, scale=None, remap_tex=False):
    """(output, gains, P) of the oracle; computed once per case, never changed."""
    t = _rig()
    out, g, pv = O.stitch_frame(list(_frames(seed)), t["sizes"], t["rois"], t["map1"], t["map2"], t["masks"], t["W"], t["H"],
                                enable_gain=True, blend=blend, seams=t["seams"] if blend else None, scale=scale, threads=8,
                                preview=preview, remap_tex=remap_tex)
    for a in (out, pv):
        a.setflags(write=False)
    return out, np.asarray(g, np.float64), pv


def _three(v):
    return np.broadcast_to(np.asarray(v, np.float32), (3,))


def _expect(P, dtype, order="rgb", scale=1.0, bias=0.0):
    """The tensor of preview bytes P (h, w, 3): this file's restatement of the definition."""
    s, b = _three(scale), _three(bias)
    planes = []
    for p in range(3):
        c = 2 - p if order == "bgr" else p
        if dtype == "u8":
            planes.append(P[..., c])
            continue
        v = P[..., c].astype(np.float32) * np.float32(s[c]) + np.float32(b[c])
        with np.errstate(over="ignore"):
            planes.append(v.astype(np.float16) if dtype == "f16" else v)
    return np.stack(planes)


def _bits(a, dtype):
    return np.ascontiguousarray(a).view(INT_OF[dtype])


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = got != want
    assert not d.any(), (what, int(d.sum()), np.argwhere(d)[:5].tolist())


def _cuda(frames):
    import torch
    return [torch.from_numpy(np.array(f)).cuda() for f in frames]  # a copy: the cached frames are read-only


def _torch_dtype(dtype):
    import torch
    return {"u8": torch.uint8, "f16": torch.float16, "f32": torch.float32}[dtype]


def _tensor(dtype, size, fill=7):
    import torch
    return torch.full((3, size[1], size[0]), fill, dtype=_torch_dtype(dtype), device="cuda")


def _yuv(W, H):
    import torch
    return torch.full((H * 3 // 2, W), 0x5A, dtype=torch.uint8, device="cuda")


def _check_tensor(got, P, dtype, what, **kw):
    _same(_bits(got.cpu().numpy(), dtype), _bits(_expect(P, dtype, **kw), dtype), what)


def _gains_same(m, g, what="gains"):
    _same(np.asarray(m.gains(), np.float64).view(np.int64), np.asarray(g, np.float64).view(np.int64), what)


def test_reference_pictures_take_every_byte_value():
    """The float rules below rest on it (every odd byte is a tie of the RNE case)."""
    t = _rig()
    P = _want(500, (t["W"], t["H"]))[2]
    assert len(np.unique(P)) == 256


# ---- 1. template size, result-frame path ----------------------------------------------------------------
@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("dtype", ["u8", "f16", "f32"])
def test_gpu_tensor_template_size(product_lib, dtype, order):
    import torch
    ox = product_lib
    t = _rig()
    size = (t["W"], t["H"])
    m = ox.Mapper(_template(ox, t), t["sizes"], blend=0, enable_gain=True)
    assert m.info()["tensor_resized"] == 0
    ten, out = _tensor(dtype, size), _yuv(*size)
    scale, bias = (1 / 255.0, 0.5, 2.0), (0.25, -3.0, 0.0)
    m.stitch_tensor(_cuda(_frames(500)), ten, output=out, order=order, scale=scale, bias=bias)
    torch.cuda.synchronize()
    want, g, P = _want(500, size)
    _check_tensor(ten, P, dtype, ("tensor", dtype, order), order=order, scale=scale, bias=bias)
    _same(out.cpu().numpy(), want, "output")
    _gains_same(m, g)
    info = m.info()
    assert (info["tensor_resized"], info["tensor_gathered"], info["tensor_no_composite"]) == (1, 0, 0)
    m.stitch_tensor(_cuda(_frames(500)), ten, output=out)
    assert m.info()["tensor_resized"] == 2


# ---- 2. resized, every kind of mapper -------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blend0", "multiband", "feather", "scaled", "texture"])
def test_gpu_tensor_resized(product_lib, kind):
    import torch
    ox = product_lib
    t = _rig()
    blend = {"multiband": 16, "feather": -5}.get(kind, 0)
    scale_out = (384, 192) if kind == "scaled" else None
    tex = kind == "texture"
    m = ox.Mapper(_template(ox, t), t["sizes"], blend=blend, enable_gain=True, scale_output=scale_out or (0, 0),
                  remap="texture" if tex else "remap")
    want, g, P = _want(500, SMALL, blend=blend, scale=scale_out, remap_tex=tex)
    out = _yuv(*(scale_out or (t["W"], t["H"])))
    dev = _cuda(_frames(500))
    for dtype in ("f16", "u8"):
        ten = _tensor(dtype, SMALL)
        m.stitch_tensor(dev, ten, output=out, scale=1 / 64.0, bias=-1.5)
        torch.cuda.synchronize()
        _check_tensor(ten, P, dtype, (kind, dtype), scale=1 / 64.0, bias=-1.5)
        _same(out.cpu().numpy(), want, (kind, "output"))
        _gains_same(m, g)
    assert m.info()["tensor_resized"] == 2


def test_gpu_tensor_resized_overlay(product_lib):
    """The overlay_include rig under a multi-band blend: the overlay is copied onto the result frame, and the
    tensor is taken from the patched frame."""
    import torch
    ox = product_lib
    W, H, blend = 512, 256, 5
    rig = copy.deepcopy(R.mask_rigs()["overlay_include"])
    mt = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    tt = OR.prepare(mt, blend)
    sizes = [(640, 360)] * len(rig["inputs"]) + [(192, 128)]
    frames = [_noise_frame(w, h, 40 + i) for i, (w, h) in enumerate(sizes)]
    want, g, P = OR.expected(tt, frames, sizes, blend=blend, enable_gain=True, preview=SMALL)
    m = ox.Mapper(mt, sizes, blend=blend, enable_gain=True)
    assert m.info()["overlays"] == 1 and m.info()["overlay_groups"] > 0
    out = _yuv(W, H)
    dev = _cuda(frames)
    for dtype in ("f16", "u8"):
        ten = _tensor(dtype, SMALL)
        m.stitch_tensor(dev, ten, output=out, scale=0.5)
        torch.cuda.synchronize()
        _check_tensor(ten, P, dtype, ("overlay", dtype), scale=0.5)
        _same(out.cpu().numpy(), want, "output")
        _gains_same(m, g)


# ---- 3. gathered path -----------------------------------------------------------------------------------
def _in_format(ox, fmt, frames, sizes):
    if fmt == "nv12":
        return [ox.nv12_from_yuv420p(f, w, h) for f, (w, h) in zip(frames, sizes)]
    if fmt == "uyvy422":  # out-then-in is the identity: the stitch sees the planar frames
        return [ox.uyvy422_from_yuv420p(f, w, h) for f, (w, h) in zip(frames, sizes)]
    return list(frames)


@pytest.mark.parametrize("fmt", ["yuv420p", "nv12", "uyvy422"])
def test_gpu_tensor_gathered_frames_in_flight(product_lib, fmt):
    """prepare_preview(301, 151), three frame slots, three different frame sets back to back on three streams,
    with the YUV frame and without it."""
    import torch
    ox = product_lib
    t = _rig()
    W, H = t["W"], t["H"]
    m = ox.Mapper(_template(ox, t), t["sizes"], blend=0, enable_gain=True)
    out_fmt = "nv12" if fmt == "nv12" else "yuv420p"
    m.set_pixel_formats(fmt, out_fmt)
    m.prepare_preview(*SMALL)
    m.set_frames_in_flight(3)
    seeds = (500, 510, 520)
    dev = [_cuda(_in_format(ox, fmt, _frames(s), t["sizes"])) for s in seeds]
    streams = [torch.cuda.Stream() for _ in seeds]
    done = 0
    for with_out in (True, False):
        for dtype in ("f16", "u8"):
            tens = [_tensor(dtype, SMALL) for _ in seeds]
            outs = [_yuv(W, H) for _ in seeds]
            torch.cuda.synchronize()
            for f in range(3):
                m.stitch_tensor(dev[f], tens[f], output=outs[f] if with_out else None, stream=streams[f], scale=1 / 255.0,
                                bias=(0.0, 1.0, -1.0))
            torch.cuda.synchronize()
            done += 3
            for f, s in enumerate(seeds):
                want, g, P = _want(s, SMALL)
                _check_tensor(tens[f], P, dtype, (fmt, with_out, dtype, f), scale=1 / 255.0, bias=(0.0, 1.0, -1.0))
                got = outs[f].cpu().numpy()
                if with_out:
                    _same(ox.yuv420p_from_nv12(got, W, H) if out_fmt == "nv12" else got, want, ("output", f))
                else:
                    assert (got == 0x5A).all(), "a YUV frame that was not passed was written"
            _gains_same(m, _want(seeds[-1], SMALL)[1], "last gains")
            info = m.info()
            assert info["tensor_gathered"] == done and info["tensor_resized"] == 0
            assert info["tensor_no_composite"] == (0 if with_out else done - 6)
    # any other size goes through the one result frame: refused with frames in flight, as a preview is
    with pytest.raises(ox.OctvrError) as et:
        m.stitch_tensor(dev[0], _tensor("u8", (300, 150)), output=_yuv(W, H))
    with pytest.raises(ox.OctvrError) as ep:
        m.stitch(dev[0], _yuv(W, H), preview=torch.zeros((150, 300, 3), dtype=torch.uint8, device="cuda"))
    assert et.value.code == ep.value.code == ox.E_INVALID
    assert m.info()["tensor_gathered"] == done and m.info()["tensor_resized"] == 0


# ---- 4. no YUV frame on the result-frame path -----------------------------------------------------------
def test_gpu_tensor_resized_without_output(product_lib):
    import torch
    ox = product_lib
    t = _rig()
    m = ox.Mapper(_template(ox, t), t["sizes"], blend=16, enable_gain=True)
    want, g, P = _want(500, SMALL, blend=16)
    ten = _tensor("f32", SMALL)
    m.stitch_tensor(_cuda(_frames(500)), ten, scale=1 / 255.0)
    torch.cuda.synchronize()
    _check_tensor(ten, P, "f32", "tensor", scale=1 / 255.0)
    _gains_same(m, g)
    info = m.info()
    assert (info["tensor_resized"], info["tensor_gathered"], info["tensor_no_composite"]) == (1, 0, 0)


# ---- 5. strides -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["resized", "gathered"])
@pytest.mark.parametrize("size", [SMALL, WIDE16])
@pytest.mark.parametrize("dtype", ["u8", "f16", "f32"])
def test_gpu_tensor_strides(product_lib, dtype, size, path):
    """The tensor as a view inside a larger tensor of a sentinel: row stride w + 5, a gap between the planes, the
    base one element past an aligned address (u8: odd; f16: a 2-byte but no 4-byte boundary; f32: a 4-byte but no
    16-byte boundary).  Every element outside the three w x h windows keeps the sentinel."""
    import torch
    ox = product_lib
    t = _rig()
    w, h = size
    rs, off = w + 5, 1
    ps = rs * h + 11
    buf = torch.full((off + 3 * ps + 64,), 7, dtype=_torch_dtype(dtype), device="cuda")
    es = buf.element_size()
    assert buf.data_ptr() % 16 == 0
    ten = buf.as_strided((3, h, w), (ps, rs, 1), off)
    assert ten.data_ptr() % (4 * es) == es and ten.stride(2) == 1
    m = ox.Mapper(_template(ox, t), t["sizes"], blend=0, enable_gain=True)
    if path == "gathered":
        m.prepare_preview(w, h)
    m.stitch_tensor(_cuda(_frames(500)), ten, scale=(1 / 255.0, 1 / 128.0, 1.0), bias=0.125, order="bgr")
    torch.cuda.synchronize()
    info = m.info()
    assert (info["tensor_resized"], info["tensor_gathered"]) == ((0, 1) if path == "gathered" else (1, 0))
    P = _want(500, size)[2]
    got = _bits(buf.cpu().numpy(), dtype)
    want = _bits(np.full(buf.shape, 7, NP_OF[dtype]), dtype).copy()
    exp = _bits(_expect(P, dtype, order="bgr", scale=(1 / 255.0, 1 / 128.0, 1.0), bias=0.125), dtype)
    for p in range(3):
        for y in range(h):
            a = off + p * ps + y * rs
            want[a:a + w] = exp[p, y]
    _same(got, want, (dtype, size, path))


# ---- 6. float rules -------------------------------------------------------------------------------------
FLOAT_RULES = {
    "unit": (1 / 255.0, 0.0),
    "imagenet": (tuple(np.float32(1.0) / (np.float32(255.0) * np.float32(s)) for s in IMAGENET_STD),
                 tuple(-np.float32(mu) / np.float32(s) for mu, s in zip(IMAGENET_MEAN, IMAGENET_STD))),
    "ties": (1.0, 2048.0),      # f16 spacing 2 at 2048: every odd byte is an exact tie
    "overflow": (1e4, 0.0),     # above 65504 -> inf
    "subnormal": (1e-7, 0.0),   # below 2^-14: subnormal halves, kept
}


@pytest.mark.parametrize("rule", sorted(FLOAT_RULES))
@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_gpu_tensor_float_rules(product_lib, dtype, rule):
    import torch
    ox = product_lib
    t = _rig()
    size = (t["W"], t["H"])
    scale, bias = FLOAT_RULES[rule]
    m = ox.Mapper(_template(ox, t), t["sizes"], blend=0, enable_gain=True)
    ten = _tensor(dtype, size)
    m.stitch_tensor(_cuda(_frames(500)), ten, scale=scale, bias=bias)
    torch.cuda.synchronize()
    P = _want(500, size)[2]
    exp = _expect(P, dtype, scale=scale, bias=bias)
    if dtype == "f16":  # the reference itself shows the property the rule is about
        if rule == "ties":
            assert (exp[0][P[..., 0] == 1] == 2048).all() and (exp[0][P[..., 0] == 3] == 2052).all()
        if rule == "overflow":
            assert np.isinf(exp).any() and not np.isinf(exp).all()
        if rule == "subnormal":
            nz = exp[exp != 0]
            assert nz.size and (np.abs(nz.astype(np.float32)) < 2.0 ** -14).all()
    _same(_bits(ten.cpu().numpy(), dtype), _bits(exp, dtype), (dtype, rule))


# ---- 7. rejections --------------------------------------------------------------------------------------
def test_gpu_tensor_rejections(product_lib):
    import torch
    ox = product_lib
    t = _rig()
    W, H = t["W"], t["H"]
    w, h = SMALL
    m = ox.Mapper(_template(ox, t), t["sizes"], blend=0, enable_gain=True)
    dev = _cuda(_frames(500))
    ptrs = (C.c_void_p * len(dev))(*[x.data_ptr() for x in dev])
    pitches = (C.c_size_t * len(dev))(*[x.stride(0) for x in dev])
    out = _yuv(W, H)
    buf = torch.full((3 * h * w * 4 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    assert base % 16 == 0

    def desc(**kw):
        d = dict(dev=base, w=w, h=h, dtype=ox.TENSOR_U8, bgr=0, row_stride=w, plane_stride=w * h)
        d.update(kw)
        return ox.TensorOut(d["dev"], d["w"], d["h"], d["dtype"], d["bgr"], d["row_stride"], d["plane_stride"],
                            (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0))

    def call(tp):
        return ox.lib().octvr_mapper_stitch_tensor(m._h, ptrs, pitches, C.c_void_p(out.data_ptr()), out.stride(0), tp,
                                                   None, 0, None)

    bad = {"null tensor": None, "null dev": desc(dev=None), "dtype 3": desc(dtype=3), "dtype -1": desc(dtype=-1),
           "bgr 2": desc(bgr=2), "bgr -1": desc(bgr=-1), "w 0": desc(w=0), "h -1": desc(h=-1),
           "row stride": desc(row_stride=w - 1), "plane stride": desc(plane_stride=w * (h - 1) + w - 1),
           "f16 at an odd address": desc(dev=base + 1, dtype=ox.TENSOR_F16),
           "f32 at a 2-byte boundary": desc(dev=base + 2, dtype=ox.TENSOR_F32)}
    for what, tp in bad.items():
        assert call(C.byref(tp) if tp is not None else None) == ox.E_INVALID, what
    torch.cuda.synchronize()
    assert (buf == 0x5A).all() and (out == 0x5A).all(), "a refused call wrote something"
    info = m.info()
    assert (info["tensor_resized"], info["tensor_gathered"]) == (0, 0)
    # the mapper is still usable
    assert call(C.byref(desc())) == 0
    torch.cuda.synchronize()
    want, g, P = _want(500, SMALL)
    _same(buf[:3 * h * w].cpu().numpy().reshape(3, h, w), _expect(P, "u8"), "tensor after the refusals")
    assert (buf[3 * h * w:] == 0x5A).all()
    _same(out.cpu().numpy(), want, "output")
    _gains_same(m, g)


def test_gpu_tensor_wrapper_errors(product_lib):
    import torch
    ox = product_lib
    t = _rig()
    m = ox.Mapper(_template(ox, t), t["sizes"], blend=0, enable_gain=True)
    dev = _cuda(_frames(500))
    good = _tensor("u8", SMALL)
    for bad in (torch.zeros((SMALL[1], SMALL[0], 3), dtype=torch.uint8, device="cuda"),   # HWC
                torch.zeros((3, 8, 8), dtype=torch.int32, device="cuda"),                  # dtype
                torch.zeros((3, 8, 8), dtype=torch.uint8),                                 # host
                torch.zeros((3, 8, 16), dtype=torch.uint8, device="cuda")[:, :, ::2]):     # inner stride
        with pytest.raises(ValueError):
            m.stitch_tensor(dev, bad)
    with pytest.raises(ValueError):
        m.stitch_tensor(dev, good, order="grb")
    with pytest.raises(ValueError):
        m.stitch_tensor(dev, good, scale=(1.0, 2.0))
