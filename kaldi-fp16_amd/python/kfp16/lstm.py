"""kfp16.lstm — ctypes binding of the projected LSTM sequence operator (include/kf_lstm.h,
DESIGN §34): Kaldi's fast-lstmp-layer, forward and exact backward, on device pointers."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import KfError, core, read_f32, read_fp16, sync

# the parameter tensors in the order of the flat layout, with their shapes as stored (an affine's
# weights are [in x out]); see Lstmp.shapes
PARAM_NAMES = ("W_x", "b", "W_r", "w_ic", "w_fc", "w_oc", "W_p", "b_p")


def _raise(what):
    s = core.kf_lstmp_last_error()
    raise KfError(f"{what}: {s.decode() if s else 'unknown error'}")


class Lstmp:
    """kf_lstmp_create: input width D, cell dim C, recurrent / non-recurrent projections R / N,
    delay < 0, for calls of up to max_rows rows in up to max_seqs sequences. forward() and
    backward() are asynchronous on the library stream."""

    def __init__(self, D: int, C_: int, R: int, N: int, delay: int, max_rows: int, max_seqs: int):
        self.h = core.kf_lstmp_create(D, C_, R, N, delay, max_rows, max_seqs)
        if not self.h:
            _raise("kf_lstmp_create")
        self.D, self.C, self.R, self.N, self.delay = D, C_, R, N, delay
        self.num_params = int(core.kf_lstmp_num_params(self.h))
        self.shapes = {"W_x": (D, 4 * C_), "b": (4 * C_,), "W_r": (R, 4 * C_), "w_ic": (C_,), "w_fc": (C_,),
                       "w_oc": (C_,), "W_p": (C_, R + N), "b_p": (R + N,)}
        self.rows = 0

    # parameters --------------------------------------------------------
    def flatten(self, named: dict) -> np.ndarray:
        """The flat fp32 layout from a dict of PARAM_NAMES (shapes as self.shapes)."""
        parts = []
        for k in PARAM_NAMES:
            a = np.asarray(named[k], dtype=np.float32)
            if a.shape != self.shapes[k]:
                raise ValueError(f"{k}: shape {a.shape}, expected {self.shapes[k]}")
            parts.append(a.reshape(-1))
        return np.ascontiguousarray(np.concatenate(parts))

    def unflatten(self, flat: np.ndarray) -> dict:
        out, off = {}, 0
        for k in PARAM_NAMES:
            n = int(np.prod(self.shapes[k]))
            out[k] = flat[off:off + n].reshape(self.shapes[k])
            off += n
        return out

    def set_params(self, named: dict):
        flat = self.flatten(named)
        if core.kf_lstmp_set_params(self.h, flat.ctypes.data) != 0:
            _raise("kf_lstmp_set_params")

    def get_params(self) -> dict:
        flat = np.empty(self.num_params, np.float32)
        if core.kf_lstmp_get_params(self.h, flat.ctypes.data) != 0:
            _raise("kf_lstmp_get_params")
        return self.unflatten(flat)

    def set_clip(self, threshold: float):
        """Row-norm clip of the recurrent derivatives in backward() (0: off; 30 after create)."""
        if core.kf_lstmp_set_clip(self.h, float(threshold)) != 0:
            _raise("kf_lstmp_set_clip")

    # compute -----------------------------------------------------------
    def forward(self, x_ptr, ldx: int, seq_row0, y_ptr, ldy: int):
        """y[rows x (R+N)] from x[rows x D] (fp16 device matrices); seq_row0 int[B+1] row offsets
        of the sequences, from 0. x must stay unchanged until backward() has run."""
        so = np.ascontiguousarray(seq_row0, dtype=np.int32)
        if core.kf_lstmp_forward(self.h, x_ptr, ldx, so.ctypes.data, len(so) - 1, y_ptr, ldy) != 0:
            _raise("kf_lstmp_forward")
        self.rows = int(so[-1])

    def backward(self, dy_ptr, ldy: int, dx_ptr, ldx: int, grad_ptr):
        """The last forward's backward: dx (fp16, or None) and every parameter gradient added into
        the fp32 device array at grad_ptr (num_params values, the flat layout)."""
        if core.kf_lstmp_backward(self.h, dy_ptr, ldy, dx_ptr, ldx, grad_ptr) != 0:
            _raise("kf_lstmp_backward")

    def state(self) -> dict:
        """What the last forward stored (synchronises): c float32 [rows x C], m float16 [rows x C],
        gates float16 [rows x 4C] (activations i, f, g, o)."""
        c, m, g = C.c_void_p(), C.c_void_p(), C.c_void_p()
        if core.kf_lstmp_state(self.h, C.byref(c), C.byref(m), C.byref(g)) != 0:
            _raise("kf_lstmp_state")
        sync()
        return dict(c=read_f32(c.value, (self.rows, self.C)), m=read_fp16(m.value, (self.rows, self.C)),
                    gates=read_fp16(g.value, (self.rows, 4 * self.C)))

    def close(self):
        if getattr(self, "h", None):
            core.kf_lstmp_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
