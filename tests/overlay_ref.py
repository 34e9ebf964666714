"""Expected output of a Mapper over a template with overlays (N inputs, K overlays; camera N + k is
overlay k).  Parity unpinned: the reference omits the overlays' RGBA -> RGB conversion before copyTo
(mapper.cpp:147-151 against :270) and fails there; the behaviour defined here is the reference with that one
conversion restored (mapper.cpp:208-312).

Two constructions from the existing oracle (oracle_py):
  chain()     blend 0: orc_stitch_frame over the N inputs for the gains g, then over all N + K cameras with
              gains g + [1.0] * K (sat_u8_rne(p * 1.0f) = p, so the overlays are the un-gained tail of the copy
              chain).
  composed()  any blend: the exported pieces (YUV -> RGBA, vignette, remap, gain feed and masked gain, the
              blenders) into an RGB result, the masked overlay copies in numpy, then the resizes and RGB -> YUV.
tests/test_overlay_ref_host.py shows they agree where both apply, and that composed() with K = 0 is
orc_stitch_frame for the blenders: that licenses composed() for blend != 0.
The LUTs come from the product's template, so the include-mask arbitration is shared."""
import ctypes as C
import json

import numpy as np

import oracle_py as O


def template_arrays(mt):
    """rois, map1s, map2s, masks over the N + K cameras and the inputs' seams (None before create_masks)."""
    n, k = len(mt), mt.num_overlays
    cams = [mt.input(i) for i in range(n)] + [mt.overlay(i) for i in range(k)]
    return {"n": n, "k": k, "rois": [c[0] for c in cams], "map1": [c[1] for c in cams], "map2": [c[2] for c in cams],
            "masks": [c[3] for c in cams], "seams": [c[4] for c in cams[:n]]}


def chain(t, frames, sizes, enable_gain=True, vig=None, scale=None, preview=None, remap_tex=False, threads=8):
    """Blend 0 -> (output, gains of the N inputs[, preview])."""
    n, k = t["n"], t["k"]
    use_gain = enable_gain and n > 1
    g = [1.0] * n
    if use_gain:
        g = list(O.stitch_frame(frames[:n], sizes[:n], t["rois"][:n], t["map1"][:n], t["map2"][:n], t["masks"][:n],
                                *t["out"], enable_gain=True, vig=None if vig is None else vig[:n], remap_tex=remap_tex,
                                threads=threads)[1])
    r = O.stitch_frame(frames, sizes, t["rois"], t["map1"], t["map2"], t["masks"], *t["out"], enable_gain=use_gain,
                       gains=(g + [1.0] * k) if use_gain else None, vig=vig, scale=scale, preview=preview,
                       remap_tex=remap_tex, threads=threads)
    return (r[0], np.asarray(g, np.float64)) + tuple(r[2:])


def _sat_mul(px, g):
    """saturate_cast<uchar>(float(px) * g), round half to even."""
    v = px.astype(np.float32) * np.asarray(g, np.float32)
    out = np.rint(v)
    out[~(v > 0)] = 0
    out[v >= 255] = 255
    return out.astype(np.uint8)


def warp(frame, size, roi_maps, vig=None, remap_tex=False):
    """One camera's per-pixel path: YUV -> RGBA, vignette, remap -> ROI-sized u8x4."""
    w, h = size
    rgba = O.yuv420_to_rgba(frame, w, h)
    if vig is not None:
        rgba = _sat_mul(rgba, np.asarray(vig, np.float32)[:, :, None])
    m1, m2 = roi_maps
    if remap_tex:
        return O.fast_remap_tex_rgba(rgba, m1, m2)
    return O.remap_u8(rgba, m1, m2, float(w), float(h))


def _resize_rgb(rgb, dw, dh):
    rgb = np.ascontiguousarray(rgb)
    sh, sw = rgb.shape[:2]
    out = np.zeros((dh, dw, 3), np.uint8)
    O.lib().orc_resize_linear_cuda_u8c(O._p(rgb), sw, sh, C.c_size_t(sw * 3), 3, O._p(out), dw, dh, C.c_size_t(dw * 3))
    return out


def composed(t, frames, sizes, blend=0, enable_gain=True, vig=None, scale=None, preview=None, remap_tex=False,
             threads=8):
    """Any blend -> (output, gains of the N inputs[, preview])."""
    n, k = t["n"], t["k"]
    W, H = t["out"]
    rois, masks = t["rois"], [np.ascontiguousarray(m, np.uint8) for m in t["masks"]]
    warped = [np.ascontiguousarray(warp(frames[i], sizes[i], (t["map1"][i], t["map2"][i]),
                                        None if vig is None else vig[i], remap_tex)) for i in range(n + k)]
    g = np.ones(n)
    if enable_gain and n > 1:  # mapper.cpp:78-82; the feed, solve and apply see the N inputs only
        g = O.gain_feed(rois[:n], warped[:n], masks[:n], W, H)
        for i in range(n):
            on = masks[i] != 0
            warped[i][on] = _sat_mul(warped[i][on], np.float32(g[i]))
    result = np.zeros((H, W, 3), np.uint8)
    bl = blend if n > 1 else 0
    r = np.ascontiguousarray(np.asarray(rois[:n], np.int32).reshape(-1))
    wp = (C.c_void_p * n)(*[a.ctypes.data for a in warped[:n]])
    if bl > 0:
        seams = [np.ascontiguousarray(s, np.uint8) for s in t["seams"]]
        sp = (C.c_void_p * n)(*[a.ctypes.data for a in seams])
        rc = O.lib().orc_multiband_blend(n, O._p(r), sp, wp, O.blend_bands(bl), O._p(result), W, H, C.c_size_t(W * 3),
                                         threads)
        assert rc == 0
    elif bl < 0:
        mp = (C.c_void_p * n)(*[a.ctypes.data for a in masks[:n]])
        rc = O.lib().orc_feather_blend(n, O._p(r), mp, wp, -bl, O._p(result), W, H, C.c_size_t(W * 3))
        assert rc == 0
    for i in range(n + k):  # the copy chain (blend 0), then the overlays onto the blended result, in order
        if i < n and bl != 0:
            continue
        x, y, w, h = rois[i]
        on = masks[i] != 0
        result[y:y + h, x:x + w][on] = warped[i][:, :, :3][on]
    sw, sh = scale if scale else (W, H)
    out = O.rgb_to_yuv420(_resize_rgb(result, sw, sh) if (sw, sh) != (W, H) else result)
    if preview:
        return out, g, _resize_rgb(result, preview[0], preview[1])
    return out, g


def expected(t, frames, sizes, blend=0, **kw):
    """What a Mapper of this blend must write: chain() where it applies, else composed()."""
    if blend == 0 or t["n"] == 1:
        return chain(t, frames, sizes, **kw)
    return composed(t, frames, sizes, blend=blend, **kw)


def prepare_oracle(rig, out_w, out_h, blend=0):
    """The same arrays from the oracle's own LUT build (no device): for the host tests."""
    luts = O.lut_build(O.json_loads_rj(json.dumps(rig)), out_w, out_h)
    n = len(rig["inputs"])
    t = {"n": n, "k": len(luts) - n, "rois": [tuple(l[0]) for l in luts], "map1": [l[1] for l in luts],
         "map2": [l[2] for l in luts], "masks": [l[3] for l in luts], "seams": [None] * n, "out": (out_w, out_h)}
    if blend != 0 and n > 1:
        t["seams"] = O.create_masks(t["rois"][:n], t["masks"][:n], out_w)
    return t


def prepare(mt, blend=0):
    """template_arrays with the output size; seam masks created when the blend needs them."""
    if blend != 0 and len(mt) > 1:
        mt.create_masks(0)
    t = template_arrays(mt)
    t["out"] = tuple(mt.out_size)
    return t
