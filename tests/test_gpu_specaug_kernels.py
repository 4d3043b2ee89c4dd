"""kf_specaug_rows and kf_specaug_apply (csrc/specaug.hip) against the numpy
restatement of the rule (tests/specaug_ref.py), bit for bit: integers and fp16 bit patterns, so
there is no tolerance. Sequence lengths cover one frame, the 64-lane pass boundary (63 / 64 / 65)
and a sequence whose regions span several passes (1500 frames: 60-85 regions at m = 20, about
1000 at m = 2, z = 0.5)."""
import numpy as np
import pytest

import specaug_ref as sr

pytestmark = pytest.mark.gpu

LENS = [1, 2, 63, 64, 65, 150, 1500, 1]
SO = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
T = int(SO[-1])
D, SEED = 40, 0x5EEDC0DE12345678
GUARD = 16          # int32 / rows of sentinel on either side of what a kernel may write


def _up_i32(kf, a):
    a = np.ascontiguousarray(a, np.int32)
    buf = kf.DeviceBuffer(max(a.nbytes, 16))
    kf.check(kf.core.bridge_transfer_int32(buf.ptr, a.ctypes.data, a.size), "upload int32")
    return buf


def _read_i32(kf, ptr, n):
    return kf.read_f32(ptr, (n,)).view(np.int32)


def _rows(kf, so, T, D, Z, z, m, m_n, k, seed, step, expect_ok=True):
    """run kf_specaug_rows into a guarded buffer -> (rc, rows)"""
    buf = _up_i32(kf, np.full(T + 2 * GUARD, 0x5A5A5A5A, np.int32))
    dso = _up_i32(kf, so) if so is not None else None
    rc = kf.core.kf_specaug_rows(buf.ptr + 4 * GUARD, dso.ptr if dso else None, len(so) - 1 if so is not None else 1, T, D, Z,
                                 float(z), m, m_n, k, seed, step)
    if expect_ok:
        kf.check(rc, "kf_specaug_rows")
    got = _read_i32(kf, buf.ptr, T + 2 * GUARD)
    assert np.all(got[:GUARD] == 0x5A5A5A5A) and np.all(got[-GUARD:] == 0x5A5A5A5A), "wrote outside [0, T)"
    return rc, got[GUARD:-GUARD]


@pytest.mark.parametrize("m,z", [(20, 0.2), (2, 0.5), (10, 0.0)])
@pytest.mark.parametrize("f", [0.5, 0.0, 1.0])
def test_rows_equal_the_reference(gpu, m, z, f):
    Z, m_n = sr.max_bins(D, f), sr.max_kept(m, z)
    for step in (0, 2 ** 32 - 1):
        _, got = _rows(gpu, SO, T, D, Z, z, m, m_n, 0, SEED, step)
        ref = sr.specaug_rows(SEED, step, 0, SO, D, Z, z, m, m_n)
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, (step, bad[:8], got[bad[:8]], ref[bad[:8]])
        if z == 0:
            assert not np.any(got == -1)
        if f == 0:
            assert np.all((got == -1) | (got >> 16 == 0))


def test_rows_one_sequence_ordinals_and_long_kept_runs(gpu):
    kf = gpu
    Z = sr.max_bins(D, 0.5)
    # B = 1 with a NULL offset pointer, and B = 1 with offsets: one sequence [0, T)
    ref = sr.specaug_rows(SEED, 5, 0, [0, T], D, Z, 0.2, 20, 80)
    _, a = _rows(kf, None, T, D, Z, 0.2, 20, 80, 0, SEED, 5)
    _, b = _rows(kf, np.array([0, T], np.int32), T, D, Z, 0.2, 20, 80, 0, SEED, 5)
    assert np.array_equal(a, ref) and np.array_equal(b, ref)
    # two ordinals give different rows, each its reference's
    _, c = _rows(kf, SO, T, D, Z, 0.2, 20, 80, 1, SEED, 5)
    _, d = _rows(kf, SO, T, D, Z, 0.2, 20, 80, 0, SEED, 5)
    assert not np.array_equal(c, d)
    assert np.array_equal(c, sr.specaug_rows(SEED, 5, 1, SO, D, Z, 0.2, 20, 80))
    # a tiny z: kept runs up to 2^31 - 1 frames, clipped at the sequence's end (the saturating sum)
    m_n = sr.max_kept(20, 1e-9)
    assert m_n == 2 ** 31 - 1
    _, e = _rows(kf, SO, T, D, Z, 1e-9, 20, m_n, 0, SEED, 1)
    assert np.array_equal(e, sr.specaug_rows(SEED, 1, 0, SO, D, Z, 1e-9, 20, m_n))
    # an odd dim and the widest one
    for dim in (43, 32767):
        Zd = sr.max_bins(dim, 1.0)
        _, g = _rows(kf, SO, T, dim, Zd, 0.2, 20, 80, 0, SEED, 2)
        assert np.array_equal(g, sr.specaug_rows(SEED, 2, 0, SO, dim, Zd, 0.2, 20, 80))


def test_rows_rejects(gpu):
    kf = gpu
    ok = dict(T=T, D=D, Z=20, z=0.2, m=20, m_n=80, k=0, seed=SEED, step=0)
    for kw in (dict(T=0), dict(D=0), dict(D=32768), dict(Z=-1), dict(Z=D + 1), dict(z=1.0), dict(z=-0.1), dict(z=float("nan")),
               dict(m=0), dict(m_n=0), dict(step=-1), dict(step=2 ** 32), dict(k=2 ** 30)):
        a = dict(ok)
        a.update(kw)
        buf = kf.DeviceBuffer(4 * T + 64)
        rc = kf.core.kf_specaug_rows(buf.ptr, None, 1, a["T"], a["D"], a["Z"], a["z"], a["m"], a["m_n"], a["k"], a["seed"], a["step"])
        assert rc == -1, kw
        assert b"kf_specaug_rows" in kf.core.kf_last_error()
    assert kf.core.kf_specaug_rows(None, None, 1, T, D, 20, 0.2, 20, 80, 0, SEED, 0) == -1
    assert kf.core.kf_specaug_rows(kf.DeviceBuffer(4 * T).ptr, None, -1, T, D, 20, 0.2, 20, 80, 0, SEED, 0) == -1
    kf.core.kf_last_error()


def _input(rows, ld, seed=3):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, ld)) * 2).astype(np.float16)
    flat = x.reshape(-1)
    for i, v in enumerate((-1.0, np.nan, np.inf, -np.inf, -0.0)):   # specials spread over the tensor
        flat[i::11][::5] = np.float16(v)
    return x


def _bands(rows, dim, seed=4):
    """per row: -1, count 0, count = dim, a band at column 0, one ending at dim, or a random one"""
    rng = np.random.default_rng(seed)
    rb = np.empty(rows, np.int32)
    for r in range(rows):
        kind = r % 7
        if kind == 0:
            rb[r] = -1
        elif kind == 1:
            rb[r] = int(rng.integers(0, dim + 1))                  # count 0 at any start
        elif kind == 2:
            rb[r] = dim << 16                                      # count = dim
        elif kind == 3:
            rb[r] = int(rng.integers(1, dim + 1)) << 16            # at column 0
        elif kind == 4:
            c = int(rng.integers(1, dim + 1))
            rb[r] = (dim - c) | (c << 16)                          # ending at dim
        else:
            c = int(rng.integers(0, dim + 1))
            rb[r] = int(rng.integers(0, dim - c + 1)) | (c << 16)
    return rb


@pytest.mark.parametrize("dim,ldx,ldy", [(40, 40, 40), (40, 48, 48), (40, 48, 40), (43, 43, 43), (43, 48, 45), (1, 1, 1),
                                         (8, 8, 16)])
@pytest.mark.parametrize("rows", [1, 517])
def test_apply(gpu, dim, ldx, ldy, rows):
    kf = gpu
    x = _input(rows + GUARD, ldx)
    rb = _bands(rows, dim)
    if rows == 1:
        rb[0] = (dim // 3) | ((dim - dim // 3) << 16)
    want = sr.specaug_apply(x[:rows, :dim], rb).view(np.uint16)
    kept = want == x[:rows, :dim].view(np.uint16)
    assert rows == 1 or (kept.any() and (~kept).any())
    dx, drb = kf.upload_fp16(x), _up_i32(kf, rb)
    ysent = np.full((rows + GUARD, ldy), 0x7B7B, np.uint16)
    dy = kf.upload_fp16(ysent.view(np.float16))
    kf.check(kf.core.kf_specaug_apply(dx.ptr, ldx, dy.ptr, ldy, rows, dim, drb.ptr), "kf_specaug_apply")
    got = kf.read_fp16(dy.ptr, (rows + GUARD, ldy)).view(np.uint16)
    assert np.array_equal(got[:rows, :dim], want)
    assert np.all(got[:rows, dim:] == 0x7B7B) and np.all(got[rows:] == 0x7B7B), "wrote outside [rows x dim]"
    assert np.array_equal(kf.read_fp16(dx.ptr, x.shape).view(np.uint16), x.view(np.uint16))   # the input is untouched
    # in place
    kf.check(kf.core.kf_specaug_apply(dx.ptr, ldx, dx.ptr, ldx, rows, dim, drb.ptr), "kf_specaug_apply")
    got = kf.read_fp16(dx.ptr, x.shape).view(np.uint16)
    assert np.array_equal(got[:rows, :dim], want)
    assert np.array_equal(got[:rows, dim:], x[:rows, dim:].view(np.uint16)) and np.array_equal(got[rows:], x[rows:].view(np.uint16))


def test_apply_specials_and_unaligned_pointer(gpu):
    """-1.0, NaN and Inf come out +0 where zeroed and untouched where kept; a pointer that is not
    16-byte aligned takes the element path"""
    kf = gpu
    dim, rows = 40, 6
    x = np.zeros((rows + 1, dim), np.float16)
    x[:, 0::3], x[:, 1::3], x[:, 2::3] = np.float16(-1.0), np.float16(np.nan), np.float16(np.inf)
    rb = np.array([-1, 5 | (20 << 16), 0, 0 | (40 << 16), 39 | (1 << 16), 0 | (1 << 16)], np.int32)
    want = sr.specaug_apply(x[:rows], rb).view(np.uint16)
    assert np.all(want[0] == 0) and np.all(want[1, 5:25] == 0) and np.array_equal(want[2], x[2].view(np.uint16))
    assert want[1, 4] == x[1, 4].view(np.uint16) and want[1, 25] == x[1, 25].view(np.uint16)
    drb = _up_i32(kf, rb)
    for shift in (0, 1):                                     # elements: 0 -> 16-byte path, 1 -> element path
        dx = kf.upload_fp16(np.concatenate([np.zeros(shift, np.float16), x.reshape(-1)]))
        dy = kf.upload_fp16(np.full(shift + x.size, 7.0, np.float16))
        kf.check(kf.core.kf_specaug_apply(dx.ptr + 2 * shift, dim, dy.ptr + 2 * shift, dim, rows, dim, drb.ptr), "kf_specaug_apply")
        got = kf.read_fp16(dy.ptr, (shift + x.size,)).view(np.uint16)
        assert np.array_equal(got[shift:shift + rows * dim].reshape(rows, dim), want), shift
        assert np.all(got[:shift] == np.float16(7.0).view(np.uint16)) and np.all(got[shift + rows * dim:] == np.float16(7.0).view(np.uint16))


def test_apply_rejects(gpu):
    kf = gpu
    b = kf.DeviceBuffer(4096)
    assert kf.core.kf_specaug_apply(b.ptr, 40, b.ptr, 40, 4, 0, b.ptr) == -1
    assert kf.core.kf_specaug_apply(b.ptr, 39, b.ptr, 40, 4, 40, b.ptr) == -1
    assert kf.core.kf_specaug_apply(b.ptr, 40, b.ptr, 39, 4, 40, b.ptr) == -1
    assert kf.core.kf_specaug_apply(None, 40, b.ptr, 40, 4, 40, b.ptr) == -1
    assert kf.core.kf_specaug_apply(b.ptr, 40, b.ptr, 40, 4, 40, None) == -1
    assert kf.core.kf_specaug_apply(b.ptr, 40, b.ptr, 40, -1, 40, b.ptr) == -1
    assert b"kf_specaug_apply" in kf.core.kf_last_error()
    assert kf.core.kf_specaug_apply(b.ptr, 40, b.ptr, 40, 0, 40, b.ptr) == 0
