"""The per-device launch configuration (csrc/launchcfg.h) on the device: kernels that need more than 64 KiB of dynamic LDS, or a grid sized
by occupancy x CU count, must behave on a second device and under a second host thread exactly as on the first.  Both tests pin that
behaviour (bit-equal outputs); neither tries to make a launch fail.

The post-processing calls take one candidate per anchor, and a 64 x 64 input has 84 anchors: there every launch of the flagged-tile path
is issued (k_heavy_rows with its LDS cap included) but no tile is above the 256 candidates that give it work.  So each decode call
runs on a 64 x 64 head and on a 128 x 128 head (336 anchors, every one a candidate)."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

from oracle.yolo11_obb import Yolo11OBB
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import ops as o
    return o


@pytest.fixture(scope="module")
def net():
    return Yolo11OBB("n", nc=12, ch=3, seed=0)


def _tiles(B=2, px=64):
    return torch.as_tensor(np.random.default_rng(11).integers(0, 256, (B, px, px, 3), dtype=np.uint8))


def _heads(ops, dev):
    """B=2 synthetic heads at 64 and 128 px with every anchor far above the confidence threshold"""
    out = []
    for px in (64, 128):
        A = ops.model_info(px, px, dev)["anchors"]
        g = torch.Generator().manual_seed(px)
        head = torch.randn((2, A, 80), generator=g)
        head[..., :64] *= 2.0
        head[..., 64:76] += 3.0
        head[..., 76] *= 0.5
        out.append((px, head))
    return out


def _run_all(ops, net, dev):
    """every call of the list on device `dev`, results on the host"""
    res = {}
    with torch.cuda.device(dev):
        d = torch.device("cuda", dev)
        ops.model_load(net.to_blob(), device=d, precision="f32")
        for px, head in _heads(ops, d):
            hd = head.to(d)
            ncand = (torch.sigmoid(hd[..., 64:76]).amax(-1) > 0.25).sum(1)
            assert int(ncand.min()) == hd.shape[1] and (px == 64 or int(ncand.min()) > 256)
            for full in (False, True):
                det, cnt = ops.decode_nms(hd, px, px, 0.25, 0.7, 300, full=full)
                res[f"decode_nms{'_full' if full else ''}_{px}"] = (det.cpu(), cnt.cpu())
        boxes, cls, conf, _ = synth.make_dets(3, 600, extent=600.0, dup_frac=0.6)  # > 512 rows: the sparse / dense scan forms, not the one-segment kernel
        order, keep, nk = ops.merge_detections(torch.as_tensor(boxes).to(d), torch.as_tensor(cls).to(d), torch.as_tensor(conf).to(d), 0.4)
        res["merge"] = (order.cpu(), keep.cpu(), nk.cpu())
        g = torch.Generator().manual_seed(5)
        x = torch.randn((1, 13, 13, 16), generator=g).to(torch.bfloat16).to(d)
        cat = ops.sppf_pools_fwd_bf16(x)
        dcat = torch.randn((1, 13, 13, 64), generator=g).to(torch.bfloat16).to(d)
        res["sppf_bwd"] = (ops.sppf_pools_bwd_bf16(cat, dcat).cpu(),)
        res["forward"] = (ops.forward(_tiles().to(d)).cpu(),)
        torch.cuda.synchronize()
    return res


def test_second_device_computes_what_the_first_does(ops, net):
    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs two devices in one process, torch.cuda.device_count() = {torch.cuda.device_count()}")
    first = _run_all(ops, net, 0)
    second = _run_all(ops, net, 1)
    assert int(first["merge"][2]) < 600 and int(first["decode_nms_128"][1].min()) > 0
    for k in first:
        for a, b in zip(first[k], second[k]):
            assert torch.equal(a, b), k


def _own_context(ops, lib, blob):
    """a context of its own on cuda:0 with the fp32 model loaded (an obb_ctx serves one host thread at a time)"""
    from oriented_object_detection_amd import _lib
    h = C.c_void_p()
    _lib.check(lib.obb_ctx_create(0, C.byref(h)))
    _lib.check(lib.obb_set_option(h, b"precision", ops.PRECISIONS["f32"]), h)
    for k in ops.MODEL_OPTIONS:  # what ops.model_load sets: every fused form on, the retired `fuse` off
        _lib.check(lib.obb_set_option(h, k.encode(), 0 if k == "fuse" else 1), h)
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    _lib.check(lib.obb_model_load(h, buf, len(blob)), h)
    return h


def test_two_host_threads_compute_what_one_does(ops, net):
    from oriented_object_detection_amd import _lib
    lib = _lib.lib()
    blob = net.to_blob()
    with torch.cuda.device(0):
        x = _tiles().cuda()
        ctxs = [_own_context(ops, lib, blob) for _ in range(2)]
        streams = [torch.cuda.Stream() for _ in range(2)]
        a = C.c_int32()
        _lib.check(lib.obb_model_info(ctxs[0], 64, 64, None, None, C.byref(a), None), ctxs[0])
        A = a.value  # 8 x 8 + 4 x 4 + 2 x 2
        assert A == 84
        heads = [torch.zeros((2, A, 80), dtype=torch.float32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        start = threading.Barrier(2, timeout=60)
        rcs = [None, None]

        def work(i):
            torch.cuda.set_device(0)
            start.wait()
            rcs[i] = lib.obb_forward(ctxs[i], C.c_void_p(x.data_ptr()), 2, 64, 64, C.c_void_p(heads[i].data_ptr()), C.c_void_p(streams[i].cuda_stream))

        th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        torch.cuda.synchronize()
        try:
            for i in range(2):
                _lib.check(rcs[i], ctxs[i])
            ops.model_load(blob, precision="f32")
            one = ops.forward(x)
            assert tuple(one.shape) == (2, A, 80)
            assert torch.equal(heads[0], one) and torch.equal(heads[1], one)
        finally:
            for h in ctxs:
                lib.obb_ctx_destroy(h)
