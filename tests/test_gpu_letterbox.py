"""k_letterbox and k_gather_tiles (csrc/decode.hip), byte for byte against oracle/postproc.py, at thin and strongly scaled crops.

LetterBox(auto=True) pads only to the next multiple of 32, so the 10-px border crops of a 642 x 640 image become 32 x 416 / 416 x 32 network
inputs (the shapes of forward_obs.SHAPE_TABLE).  Every crop is cut at a non-zero, odd offset out of a larger random image, so a read one
pixel outside the crop changes the result; every output is written into a guarded buffer.

Crops whose shorter side would round to ZERO pixels (1 x 416 at imgsz 128: round(1 * 128 / 416) = 0) are outside LetterBox's domain (cv2
rejects an empty resize) and are not cases here.

k_gather_tiles stores 4 bytes per thread: with a row pitch tile * C that is no multiple of 4 (tile 5 or 127 at C = 3, tile 1) every row but
the first starts misaligned, and those shapes go through the byte path."""
import numpy as np
import pytest
import torch

import bounds
from oracle import postproc as pp

pytestmark = pytest.mark.gpu

OFF_X, OFF_Y = 37, 53
CROPS = [(10, 416), (416, 10), (1, 416), (416, 1), (2, 2), (10, 8), (3, 500), (1000, 50), (175, 263), (900, 1100)]  # (h, w)
NETWORK_SHAPE_416 = {(10, 416): (32, 416), (416, 10): (416, 32), (1, 416): (32, 416), (416, 1): (416, 32), (3, 500): (32, 416),
                     (1000, 50): (416, 32), (10, 8): (416, 352), (2, 2): (416, 416), (175, 263): (288, 416), (900, 1100): (352, 416)}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops as o
    return o


@pytest.fixture(scope="module")
def images():
    out = {}
    for C in (3, 4):
        img = np.random.default_rng(40 + C).integers(0, 256, (OFF_Y + 1000 + 7, OFF_X + 1100 + 5, C), dtype=np.uint8)
        out[C] = (img, torch.as_tensor(img).cuda())
    return out


@pytest.mark.parametrize("imgsz", [416, 128])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("ch,cw", CROPS, ids=lambda v: str(v))
def test_letterbox_byte_for_byte(ops, images, ch, cw, C, imgsz):
    img, dimg = images[C]
    p = pp.letterbox_params(ch, cw, imgsz)
    if min(p["new_w"], p["new_h"]) < 1:
        assert imgsz == 128 and (ch, cw) in ((1, 416), (416, 1))  # the only two: nothing else may drop out
        return
    if imgsz == 416:
        assert (p["out_h"], p["out_w"]) == NETWORK_SHAPE_416[ch, cw], p
    assert p["out_h"] % 32 == 0 and p["out_w"] % 32 == 0
    assert p["resize"] == ((ch, cw) not in ((10, 416), (416, 10), (1, 416), (416, 1)) or imgsz != 416)
    x, y = OFF_X, OFF_Y
    exp, _ = pp.letterbox(np.ascontiguousarray(img[y:y + ch, x:x + cw]), imgsz)
    assert exp.shape == (p["out_h"], p["out_w"], C)
    q = ops.letterbox_shape(ch, cw, imgsz)
    assert (q["out_h"], q["out_w"]) == (p["out_h"], p["out_w"])
    g = bounds.Guarded(exp.shape, torch.uint8)
    torch.ops.obbhip.letterbox(dimg, x, y, x + cw, y + ch, imgsz, g.out)
    torch.cuda.synchronize()
    assert g.guards_intact(), "write outside the output"
    got = g.out.cpu().numpy()
    assert np.array_equal(got, exp), (int((got != exp).sum()), np.argwhere(got != exp)[:3].tolist())
    # the convenience wrapper allocates the same shape and gives the same bytes
    out, _ = ops.letterbox(dimg, x, y, x + cw, y + ch, imgsz)
    assert np.array_equal(out.cpu().numpy(), exp)


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("tile", [1, 5, 127, 128])
def test_gather_tiles_byte_for_byte(ops, tile, C):
    H, W = 301, 311
    img = np.random.default_rng(tile + C).integers(0, 256, (H, W, C), dtype=np.uint8)
    xy = [(1, 3), (W - tile - 1, 7), (33, H - tile), (W - tile, H - tile), (0, 0)]  # odd offsets; the last pixel of the image; the first
    rects = np.array([(x, y, x + tile, y + tile) for x, y in xy], np.int32)
    assert (tile * C % 4 != 0) == ((tile, C) in ((1, 3), (5, 3), (127, 3)))
    g = bounds.Guarded((len(xy), tile, tile, C), torch.uint8)
    torch.ops.obbhip.gather_tiles(torch.as_tensor(img).cuda(), torch.as_tensor(rects).cuda(), tile, g.out)
    torch.cuda.synchronize()
    assert g.guards_intact(), "write outside the output"
    got = g.out.cpu().numpy()
    for t, (x, y) in enumerate(xy):
        assert np.array_equal(got[t], img[y:y + tile, x:x + tile]), (tile, C, t)
    assert np.array_equal(ops.gather_tiles(torch.as_tensor(img).cuda(), torch.as_tensor(rects).cuda(), tile).cpu().numpy(), got)
