"""`upacc` splits the [cout][cin] matrix of the 1x1 behind [Upsample x2 | skip] by columns: [0, up_c) packed for k_pw_f32 (the coarse launch),
[up_c, cin) for the two-fragment k_conv_f32 form (the fine launch).  Unpacked through the kernels' documented lane layouts, the two parts must
reproduce the unsplit packing of the one-launch form -- every output channel's k sequence (16-channel pieces in ascending order, lane group g,
element s), weight for weight -- for the n and s widths.  Host code only: no device."""
import ctypes as C

import numpy as np
import pytest

SHAPES = {"n": ((128, 256, 128), (64, 128, 128)), "s": ((256, 512, 256), (128, 256, 256))}  # (cout, up_c, skip_c) of model.13.cv1 / model.16.cv1


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g._load_build_module().build()
    import oriented_object_detection_amd  # noqa: F401
    from oriented_object_detection_amd import _lib
    return _lib.lib()


def _pack(L, form, w, c0, nc):
    cout, cin = w.shape
    need, til = C.c_int64(), (C.c_int32 * 3)()
    wp = w.ctypes.data_as(C.c_void_p)
    assert L.obb_debug_pack_1x1(form, wp, cout, cin, c0, nc, None, 0, C.byref(need), til) == 0
    out = np.empty(need.value, np.float32)
    assert L.obb_debug_pack_1x1(form, wp, cout, cin, c0, nc, out.ctypes.data_as(C.c_void_p), out.size, C.byref(need), til) == 0
    return out, tuple(til)


def _unpack_conv32(pk, cout, k, CK, WC, NC):
    """[cout block][stage][fragment]{[piece][lane][4]} -> [cout][k] with k = 16 * (stage * pieces + piece) + 4 * g + s"""
    nfb, kst, nstage = WC * NC, CK // 16, k // CK
    m = np.full((cout, k), np.nan, np.float32)
    a = pk.reshape(-1, nstage, nfb, kst, 64, 4)
    for cb in range(a.shape[0]):
        for f in range(nfb):
            for lane in range(64):
                r, g = lane & 15, lane >> 4
                co = cb * nfb * 16 + (32 * (f >> 1) + (r >> 2) * 8 + (f & 1) * 4 + (r & 3) if NC == 2 else 16 * f + r)
                if co >= cout:
                    assert not a[cb, :, f, :, lane].any()
                    continue
                for st in range(nstage):
                    for p in range(kst):
                        k0 = 16 * (st * kst + p) + 4 * g
                        m[co, k0:k0 + 4] = a[cb, st, f, p, lane]
    return m


def _unpack_pw32(pk, cout, k):
    """[cout block of 64][piece][fragment 4][lane][4] -> [cout][k]"""
    a = pk.reshape(cout // 64, k // 16, 4, 64, 4)
    m = np.full((cout, k), np.nan, np.float32)
    for cb in range(a.shape[0]):
        for f in range(4):
            for lane in range(64):
                r, g = lane & 15, lane >> 4
                co = cb * 64 + 16 * (r >> 2) + 4 * f + (r & 3)
                for p in range(k // 16):
                    m[co, 16 * p + 4 * g:16 * p + 4 * g + 4] = a[cb, p, f, lane]
    return m


@pytest.mark.parametrize("scale", ["n", "s"])
def test_column_split_reproduces_the_unsplit_packing(L, scale):
    for i, (cout, up_c, sk) in enumerate(SHAPES[scale]):
        w = np.random.default_rng(10 * i + len(scale)).standard_normal((cout, up_c + sk)).astype(np.float32)
        whole, (ck2, wc2, nc2) = _pack(L, 2, w, 0, up_c + sk)
        coarse, _ = _pack(L, 0, w, 0, up_c)
        fine, (ck1, wc1, nc1) = _pack(L, 1, w, up_c, sk)
        assert up_c % ck2 == 0 and sk % ck1 == 0 and (wc1, nc1) == (2, 2)  # a stage never straddles the two members; the fine form is the two-fragment one
        mw = _unpack_conv32(whole, cout, up_c + sk, ck2, wc2, nc2)
        assert np.array_equal(mw, w)  # (the unsplit packing holds every weight at its k position)
        assert np.array_equal(_unpack_pw32(coarse, cout, up_c), mw[:, :up_c])
        assert np.array_equal(_unpack_conv32(fine, cout, sk, ck1, wc1, nc1), mw[:, up_c:])
        assert coarse.size == cout * up_c  # no padding, nothing but the split columns
