"""Device-side helpers of the direct kernel tests (test_gpu_layer_kernels.py,
test_gpu_ivector_kernels.py): raw-bit uploads and reads, padded and poisoned buffers, and the
rejection check. `kf` is the kfp16 module the `gpu` fixture returns."""
import ctypes as C

import numpy as np
import pytest

NAN16 = 0x7F7F           # an fp16 NaN: no kernel result equals it
POISON32 = 0x7F7F7F7F    # 3.39e38 as fp32


def ints(rng, shape, lo, hi, dtype=np.float16):
    return rng.integers(lo, hi + 1, shape).astype(dtype)


def gauss(rng, shape, dtype=np.float16):
    return rng.standard_normal(shape).astype(dtype)


def iarr(v):
    return (C.c_int * max(len(v), 1))(*[int(i) for i in v])


def up_u16(kf, a):
    """upload 16-bit words as they are (fp16 values or their bit patterns)"""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 2
    return kf.upload_fp16(a.view(np.float16))


def rd_u16(kf, ptr, shape):
    return kf.read_fp16(ptr, shape).view(np.uint16)


def up_u32(kf, a):
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    return kf.upload_f32(a.view(np.float32))


def rd_u32(kf, ptr, shape):
    return kf.read_f32(ptr, shape).view(np.uint32)


def up_bytes(kf, a):
    """upload uint8 (padded to a multiple of 4 with zeros)"""
    a = np.ascontiguousarray(a, np.uint8).reshape(-1)
    p = np.zeros((len(a) + 3) // 4 * 4, np.uint8)
    p[:len(a)] = a
    return up_u32(kf, p.view(np.uint32))


def rd_bytes(kf, ptr, n):
    """n bytes of a buffer made by up_bytes"""
    return rd_u32(kf, ptr, ((n + 3) // 4,)).view(np.uint8)[:n]


def padded(a, ld, extra_rows=0, fill=NAN16):
    """a [rows x cols] fp16 inside a [rows + extra_rows x ld] image of `fill` words"""
    a = np.asarray(a, np.float16)
    img = np.full((a.shape[0] + extra_rows, ld), fill, np.uint16)
    img[:a.shape[0], :a.shape[1]] = a.view(np.uint16)
    return img


def poison16(rows, ld):
    return np.full((rows, ld), NAN16, np.uint16)


def poison32(n):
    return np.full(n, POISON32, np.uint32)


def check_padding(img, rows, cols, fill):
    """everything of the read-back image outside [rows x cols] still holds the poison"""
    assert np.all(img[:rows, cols:] == fill), "columns past the logical width were written"
    assert np.all(img[rows:] == fill), "rows past the logical height were written"


def same_bits16(got, ref):
    """fp16 results bit-identical to the reference values (given in any float type)"""
    ref16 = np.asarray(ref).astype(np.float16)
    assert np.array_equal(ref16.astype(np.float64), np.asarray(ref, np.float64)), "reference not exact in fp16"
    g = np.asarray(got).view(np.uint16) if np.asarray(got).dtype != np.uint16 else np.asarray(got)
    bad = np.flatnonzero(g.reshape(-1) != ref16.view(np.uint16).reshape(-1))
    assert bad.size == 0, (f"{bad.size} of {g.size} elements differ, first at {bad[0]}: got "
                           f"{g.reshape(-1)[bad[0]:bad[0] + 1].view(np.float16)[0]} want {ref16.reshape(-1)[bad[0]]}")


def within(got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    assert np.all(np.isfinite(np.asarray(got, np.float64)))
    worst = np.argmax(err - bound)
    assert np.all(err <= bound), (f"element {worst}: got {np.asarray(got).reshape(-1)[worst]} want "
                                  f"{np.asarray(ref).reshape(-1)[worst]} bound {np.broadcast_to(bound, err.shape).reshape(-1)[worst]}")


def rejected(kf, rc, needle, last_error="kf_layers_last_error"):
    """rc is -1, the module's error text names the cause, and check() raises with that text"""
    assert rc == -1
    msg = getattr(kf.core, last_error)()
    assert msg and needle in msg.decode(), msg
    with pytest.raises(kf.KfError) as e:
        kf.check(rc, "call")
    assert needle in str(e.value)
