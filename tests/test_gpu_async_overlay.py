"""AsyncMultiMapper over a rig with an overlay: n_inputs = N + K frames through the footprint upload, the
unpack kernels and two mappers (blend 0: the overlay in the composite LUT; multi-band: overlay_apply_kernel on
the result frame), five frames through the three pipeline slots, registered and unregistered outputs, planar
and NV12.  The device frames hold a fixed pattern outside the uploaded footprint (as in
test_gpu_async_nv12_byte_path), so an overlay tap that was used and never uploaded shows as a mismatch."""
import json

import numpy as np
import pytest

import overlay_ref as OR
import test_gpu_async_nv12 as A
import test_gpu_overlay as T

pytestmark = pytest.mark.gpu

W, H = T.W, T.H


@pytest.fixture(scope="module")
def case(product_lib):
    """The overlay_include rig as two templates (blend 0 and multi-band), five frame sets and their expected
    region outputs: the left half stitched at 256 x 256 by the first mapper, the right half by the second."""
    ox = product_lib
    rig = T.rig_one()
    sizes = T._sizes(rig)
    mts = [ox.MapperTemplate.from_json(json.dumps(rig), W, H) for _ in range(2)]
    ts = [OR.prepare(mts[0], 0), OR.prepare(mts[1], 5)]
    frames = [T._frames(sizes, 900 + 10 * f) for f in range(5)]
    want = [[OR.expected(ts[k], fr, sizes, blend=b, scale=(W // 2, H))[0] for k, b in enumerate((0, 5))]
            for fr in frames]
    return {"ox": ox, "mts": mts, "sizes": sizes, "frames": frames, "want": want}


@pytest.mark.parametrize("fmt", [("yuv420p", "yuv420p"), ("nv12", "nv12")], ids=["planar", "nv12"])
@pytest.mark.parametrize("registered", [False, True])
def test_gpu_async_overlay(case, fmt, registered):
    ox, sizes = case["ox"], case["sizes"]
    am = ox.AsyncMultiMapper(case["mts"], sizes, (W, H), [0, 5], [0, 0],
                             [(0.0, 0.0, 0.5, 1.0), (0.5, 0.0, 0.5, 1.0)])
    am.set_pixel_formats(*fmt)
    outs = [A.new_out(W, H, fmt[1]) for _ in case["frames"]]
    if registered:
        for out in outs:
            am.register_output(out)
    for fr, out in zip(case["frames"], outs):  # more frames than slots, all pushed before the first pop
        am.push([A.in_planes(f, w, h, fmt[0]) for f, (w, h) in zip(fr, sizes)], out)
    for f, out in enumerate(outs):
        assert am.pop() is out
        A.check(out, A.want_out(W, H, [(0, 0, case["want"][f][0]), (W // 2, 0, case["want"][f][1])], fmt[1]),
                (fmt, registered, f))
    am.close()


def test_gpu_async_overlay_chain_needs_equal_inputs(case):
    """gain_modes[1] = 0 with N_1 != N_0 (2 inputs + 1 overlay against 3 inputs): OCTVR_E_INVALID."""
    ox = case["ox"]
    rig = T.rig_one()
    rig["inputs"].append(rig["overlays"].pop())
    other = ox.MapperTemplate.from_json(json.dumps(rig), W, H)
    assert len(other) == 3 and other.num_overlays == 0
    with pytest.raises(ox.OctvrError) as e:
        ox.AsyncMultiMapper([case["mts"][0], other], case["sizes"], (W, H), [0, 0], [0, 0],
                            [(0.0, 0.0, 0.5, 1.0), (0.5, 0.0, 0.5, 1.0)])
    assert e.value.code == ox.E_INVALID
    am = ox.AsyncMultiMapper([case["mts"][0], other], case["sizes"], (W, H), [0, 0], [0, 1],
                             [(0.0, 0.0, 0.5, 1.0), (0.5, 0.0, 0.5, 1.0)])  # unchained: the split may differ
    am.close()
