"""Case builders of tests/test_gpu_vignette_extremes.py: rigB's cameras with vignette coefficient sets whose gain
maps tie, saturate, vanish, turn negative or infinite; the oracle's maps and stitches of them (computed once per
case and never changed); and the counts that show a case reaches what it is for, taken from the oracle and numpy
alone.  Nothing here touches the GPU except `template`, which reads the LUT back from the product's template as
the other vignette tests do."""
import copy
import functools
import json

import numpy as np

import oracle_py as O

W, H = 768, 384  # rigB's 192 x 108 cameras at this output: test_gpu_vignette.py's shape

# Constant maps are exact in f32 although a / 2^exposure is not always exact in f64: 1 / fl64(4/3) is within an
# ulp(f64) of 0.75 and rounds to it.  `constant_gain` below checks each one.  The map resized to a camera is not
# constant to the bit: the four f32 weights of cuda::resize do not always sum to 1, so some gains sit an ulp off
# (0.49999997 beside 0.5).  `counts` therefore takes ties and clamps from the resized maps, as the kernels do.
HALF = {"vignette": [2.0, 0.0, 0.0, 0.0]}                                  # 0.5: every odd value ties
THREE_QUARTERS = {"vignette": [8.0 / 3.0, 0.0, 0.0, 0.0], "exposure": 1.0}  # 0.75: values = 2 (mod 4) tie
ONE_AND_HALF = {"vignette": [2.0 / 3.0, 0.0, 0.0, 0.0]}                    # 1.5: odd values tie, > 170 clamp
QUARTER = {"vignette": [4.0, 0.0, 0.0, 0.0]}                               # 0.25: values = 2 (mod 4) tie
DOUBLE = {"vignette": [0.5, 0.0, 0.0, 0.0]}                                # 2: values > 127 clamp
DOUBLE_EV = {"vignette": [1.0, 0.0, 0.0, 0.0], "exposure": 1.0}            # 2 through the exposure
TIMES_64 = {"vignette": [1.0 / 64.0, 0.0, 0.0, 0.0]}                       # 64: values > 3 clamp, 0 stays 0
VANISHING = {"vignette": [300.0, 0.0, 0.0, 0.0]}                           # 1 / 300: products round to 0 or 1
NEGATIVE = {"vignette": [-1.0, 0.0, 0.0, 0.0]}                             # -1: every product <= 0
POLE = {"vignette": [1.0, -1.2, 0.0, 0.0]}      # zero of the denominator at r = 0.913: the map's corners
POLE_INSIDE = {"vignette": [1.0, -4.0, 0.0, 0.0]}  # zero at r = 0.5: inside rigB's crop circles (r <= 0.707)
INFINITE = {"vignette": [0.0, 0.0, 0.0, 0.0]}   # 1 / 0 = +inf everywhere: 0 * inf = NaN -> 0, the rest -> 255
STEEP = {"vignette": [1.0, 6.0, 0.0, 0.0]}      # 1 .. 1/7 over the map: neighbouring pixels' gains differ
STEEP_EV = {"vignette": [1.0, 6.0, 0.0, 0.0], "exposure": 1.5}
NONE = {}                                       # no vignette: kStageNoVig beside vignetted cameras

CONSTANT = {"half": 0.5, "three_quarters": 0.75, "one_and_half": 1.5, "quarter": 0.25, "double": 2.0, "double_ev": 2.0,
            "times_64": 64.0}

# family -> the six cameras' options.  rigB's copy chain (blend 0) shows cameras 2 to 5 only (7, 14, 15 and 65 % of
# the output; cameras 0 and 1 lie under later ones and reach the gains alone), the blends show all six: so the
# camera without a vignette is camera 2, and each family's sharpest members are cameras 3 to 5.
FAMILIES = {
    "ties": [QUARTER, THREE_QUARTERS, NONE, ONE_AND_HALF, STEEP, HALF],
    "saturation": [NEGATIVE, DOUBLE_EV, NONE, VANISHING, TIMES_64, DOUBLE],
    "pole": [INFINITE, STEEP_EV, NONE, INFINITE, POLE, POLE_INSIDE],
}

# Cameras of four sizes: the 512 x 512 map shrunk, copied 1:1, enlarged (width a multiple of 8) and shrunk
# strongly, all with steep maps so that a wrong source coordinate or a clamped last column changes bytes.
RESIZE_SIZES = [(192, 108), (64, 36), (192, 108), (64, 36), (520, 300), (512, 512)]
RESIZE_OPTIONS = [STEEP, STEEP, NONE, STEEP_EV, {"vignette": [1.0, 6.0, 0.0, 0.0], "exposure": 0.5}, STEEP]

# A vignetted camera 196 pixels wide (196 % 8 == 4: every tile that shows it is a gathered, "wide" one) beside
# 192-wide cameras with and without a vignette (staged float4 gains in the same launch).
W196_SIZES = [(192, 108)] * 4 + [(196, 108), (192, 108)]
W196_OPTIONS = [NONE, HALF, NONE, ONE_AND_HALF, STEEP, STEEP_EV]


def constant_gain(opts):
    """The value of a constant map, checked to be one value bit for bit."""
    m = O.vignette_map(opts)
    v = m.view(np.int32)
    assert (v == v[0, 0]).all()
    return float(m[0, 0])


def crop_for(w, h):
    """rigB's crop (a centred circle of the frame's height, [x0, x1, y0, y1]) for a w x h camera."""
    d = min(w, h)
    return {"rect": [(w - d) // 2, (w + d) // 2, (h - d) // 2, (h + d) // 2], "is_circular": True}


def rig_with(options, sizes=None):
    """rigB's JSON with per-camera vignette options and, where given, per-camera (w, h)."""
    rig, _ = O.load_rig("rigB")
    rig = json.loads(json.dumps(rig))
    assert len(options) == len(rig["inputs"])
    for k, (c, extra) in enumerate(zip(rig["inputs"], options)):
        o = c["options"]
        if sizes is not None:
            o["width"], o["height"] = sizes[k]
            o["crop"] = crop_for(*sizes[k])
        o.update(copy.deepcopy(extra))
    return rig


def sizes_of(rig):
    return [(c["options"]["width"], c["options"]["height"]) for c in rig["inputs"]]


def oracle_vig(rig):
    """Per camera: (the oracle's 512 x 512 map or None, that map resized to the camera's size or None)."""
    base, resized = [], []
    for c, (w, h) in zip(rig["inputs"], sizes_of(rig)):
        m = O.vignette_map(c["options"])
        base.append(m)
        resized.append(None if m is None else O.resize_linear_cuda_f32(m, w, h))
    return base, resized


_TEMPLATES = {}


def template(ox, key, rig, out_w=W, out_h=H):
    """The product's template of `rig` (create_masks(0) seams) with what the oracle needs of it, built once per
    key: {"mt", "rig", "sizes", "W", "H", "rois", "map1", "map2", "masks", "seams", "vig"}.  Asserts that the
    product's 512 x 512 vignette maps equal the oracle's bit for bit (int32 views: NaN and -0 count)."""
    if key in _TEMPLATES:
        return _TEMPLATES[key]
    mt = ox.MapperTemplate.from_json(json.dumps(rig), out_w, out_h)
    base, vig = oracle_vig(rig)
    for i, want in enumerate(base):
        got = mt.vignette(i)
        if want is None:
            assert got is None, (key, i)
            continue
        assert got is not None and got.shape == want.shape, (key, i)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (key, i)
    mt.create_masks(0)
    t = {"mt": mt, "rig": rig, "sizes": sizes_of(rig), "W": out_w, "H": out_h, "vig": vig,
         "rois": [], "map1": [], "map2": [], "masks": [], "seams": []}
    for i in range(len(mt)):
        roi, m1, m2, mk, sm = mt.input(i)
        t["rois"].append(roi); t["map1"].append(m1); t["map2"].append(m2); t["masks"].append(mk); t["seams"].append(sm)
    _TEMPLATES[key] = t
    return t


@functools.lru_cache(maxsize=None)
def random_frames(sizes, seed):
    """Random-byte YUV420P frames: every channel value occurs and YUV -> RGB itself saturates."""
    fr = tuple(O.rand_img(w, h * 3 // 2, 1, seed + i).reshape(h * 3 // 2, w) for i, (w, h) in enumerate(sizes))
    for f in fr:
        f.setflags(write=False)
    return fr


_WANT = {}


def want(key, t, frames, blend=0, vig=True, **kw):
    """The oracle's stitch_frame of template t (estimated gains), once per (key, blend, vig, kw) and read-only:
    (output, gains) or (output, gains, preview)."""
    k = (key, blend, vig, tuple(sorted(kw.items())))
    if k not in _WANT:
        r = O.stitch_frame(list(frames), t["sizes"], t["rois"], t["map1"], t["map2"], t["masks"], t["W"], t["H"],
                           enable_gain=True, blend=blend, seams=t["seams"], vig=t["vig"] if vig else None, threads=8, **kw)
        for a in r:
            a.setflags(write=False)
        _WANT[k] = r
    return _WANT[k]


def footprint(t, i):
    """Boolean (h, w) image of camera i's source pixels that some claimed output pixel taps (cv::remap's cell:
    the fixed-point coordinate's integer part and the pixel right of and below it, inside the image)."""
    w, h = t["sizes"][i]
    m1, m2, mk = t["map1"][i], t["map2"][i], t["masks"][i]
    with np.errstate(invalid="ignore"):
        fx, fy = m1 * np.float32(w) * np.float32(32), m2 * np.float32(h) * np.float32(32)
        ok = (mk != 0) & np.isfinite(fx) & np.isfinite(fy) & (np.abs(fx) < 2.0 ** 30) & (np.abs(fy) < 2.0 ** 30)
    sx = np.rint(np.where(ok, fx, 0)).astype(np.int64) >> 5
    sy = np.rint(np.where(ok, fy, 0)).astype(np.int64) >> 5
    fp = np.zeros((h, w), bool)
    for dx in (0, 1):
        for dy in (0, 1):
            x, y = sx + dx, sy + dy
            k = ok & (x >= 0) & (x < w) & (y >= 0) & (y < h)
            fp[y[k], x[k]] = True
    return fp


def products(t, frames, i):
    """float32(c) * g of camera i's R, G, B over its footprint: an (n, 3) f32 array, as vig_mul forms them."""
    w, h = t["sizes"][i]
    rgb = O.yuv420_to_rgba(np.ascontiguousarray(frames[i]), w, h)[..., :3].astype(np.float32)
    fp = footprint(t, i)
    with np.errstate(invalid="ignore", over="ignore"):
        return rgb[fp] * t["vig"][i][fp][:, None]


def counts(t, frames):
    """Over the footprints of the rig's vignetted cameras: products that are exact ties (frac == 0.5, below the
    clamp), products >= 255.5 (clamped), and gains that are negative or not finite."""
    ties = clamped = odd_gains = 0
    for i, v in enumerate(t["vig"]):
        if v is None:
            continue
        p = products(t, frames, i)
        with np.errstate(invalid="ignore"):
            ties += int(((p > 0) & (p < 255) & (p - np.floor(p) == np.float32(0.5))).sum())
            clamped += int((p >= np.float32(255.5)).sum())
        g = v[footprint(t, i)]
        with np.errstate(invalid="ignore"):
            odd_gains += int((~np.isfinite(g) | (g < 0)).sum())
    return {"ties": ties, "clamped": clamped, "odd_gains": odd_gains}


def sat_u8(p):
    """saturate_cast<uchar>(float) of an array: round half to even, clamp, NaN -> 0."""
    with np.errstate(invalid="ignore"):
        return np.where(p > 0, np.rint(np.minimum(p, np.float32(255))), 0).astype(np.uint8)


def neighbour_changes(t, frames):
    """Channel values over the vignetted cameras' footprints whose byte would differ with the gain of the pixel
    to the right: what a gain map shifted by one pixel changes."""
    n = 0
    for i, v in enumerate(t["vig"]):
        if v is None:
            continue
        w, h = t["sizes"][i]
        rgb = O.yuv420_to_rgba(np.ascontiguousarray(frames[i]), w, h)[..., :3].astype(np.float32)
        fp = footprint(t, i)[:, :-1]
        with np.errstate(invalid="ignore", over="ignore"):
            a = sat_u8(rgb[:, :-1] * v[:, :-1, None])[fp]
            b = sat_u8(rgb[:, :-1] * v[:, 1:, None])[fp]
        n += int((a != b).sum())
    return n


def changed_fraction(a, b, out_h):
    """Fraction of the output's luma pixels that differ between two YUV420P frames."""
    return float((np.asarray(a)[:out_h] != np.asarray(b)[:out_h]).mean())


def unaligned(frames, sizes):
    """Each frame inside a (rows, w + 2) byte tensor from flat offset 2: base pointer + 2, pitch w + 2."""
    import torch
    dev = []
    for f, (w, h) in zip(frames, sizes):
        rows = h * 3 // 2
        buf = torch.full(((rows + 1) * (w + 2),), 0xA5, dtype=torch.uint8, device="cuda")
        v = buf[2:2 + rows * (w + 2)].view(rows, w + 2)[:, :w]
        v.copy_(torch.from_numpy(np.array(f)).cuda())  # a copy: the cached frames are read-only
        assert v.data_ptr() % 8 == 2 and v.stride(0) == w + 2
        dev.append(v)
    return dev
