"""kfp16 — Python binding of the MI355X kaldi-fp16 core.

Thin ctypes layer over the C-ABI libraries built in ``kaldi-fp16_amd/lib``:
``libkaldi_fp16.so`` (bridge_* / ops_* / chain_* / den_* / kf_* kernels) and
``libkaldi_fp16_nnet.so`` (the C++ host layer restating internal/nnet).
Tests and bench.py drive the product through this module; nothing here
computes anything itself. If the HIP libraries are missing, importing this
module raises — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# KFP16_LIBDIR: load another in-tree build (A/B timing of kernel variants)
LIBDIR = os.environ.get("KFP16_LIBDIR") or os.path.normpath(os.path.join(_HERE, "..", "..", "lib"))
INCDIR = os.path.normpath(os.path.join(_HERE, "..", "..", "..", "include"))


class KfError(RuntimeError):
    pass


def _load(name):
    path = os.path.join(LIBDIR, name)
    if not os.path.exists(path):
        raise ImportError(
            f"kfp16: {path} is missing — build the HIP libraries first "
            "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
    if os.environ.get("KF_ERR_TRACE", "0") not in ("", "0"):
        return _TracedCDLL(path, mode=C.RTLD_GLOBAL)
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


# KF_ERR_TRACE=1: origin of a HIP error left pending. Every call through the
# libraries peeks at HIP's pending error (kf_peek_error, not consumed) before and after it:
# one pending before the call was raised by HIP calls the process made outside kfp16 since
# its previous call (torch, ctypes users); one pending after it by the call itself. Notes
# go to stderr and to trace_notes; the libraries' own kf_take_pending checks are unchanged.
trace_notes: list = []


def _trace_note(msg):
    import sys
    import traceback
    where = "".join(traceback.format_stack(limit=5)[:-2]).rstrip()
    trace_notes.append(msg + "\n" + where)
    print(f"kfp16 KF_ERR_TRACE: {msg}\n{where}", file=sys.stderr, flush=True)


class _TracedCDLL(C.CDLL):
    def __init__(self, path, mode):
        super().__init__(path, mode=mode)
        peek = C.CDLL(os.path.join(LIBDIR, "libkaldi_fp16.so"), mode=mode).kf_peek_error
        peek.restype, peek.argtypes = C.c_int, []
        base = self._FuncPtr

        class _Traced(base):
            _flags_ = base._flags_
            _restype_ = base._restype_

            def __call__(self, *args):
                pre = peek()
                if pre:
                    _trace_note(f"HIP error {pre} pending before {self.__name__} "
                                "(raised outside kfp16 since its previous call)")
                r = base.__call__(self, *args)
                post = peek()
                if post and post != pre:
                    _trace_note(f"HIP error {post} pending after {self.__name__}")
                return r

        self._FuncPtr = _Traced


core = _load("libkaldi_fp16.so")
nnet = _load("libkaldi_fp16_nnet.so")

_vp, _i, _f, _ll, _sz = C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.c_size_t


def _sig(lib, name, res, *args):
    if os.environ.get("KFP16_LIBDIR") and not hasattr(lib, name):
        return None  # A/B against an older build that lacks this entry point
    fn = getattr(lib, name)
    fn.restype = res
    fn.argtypes = list(args)
    return fn


# ---------------------------------------------------------------- bridge_*
for _n in ("bridge_last_error", "ops_last_error", "kf_last_error", "nnet_last_error"):
    _sig(core if not _n.startswith("nnet") else nnet, _n, C.c_char_p)
_sig(core, "bridge_clear_error", None)
_sig(core, "kf_take_pending", _i, C.c_char_p)
_sig(core, "kf_pending_log", C.c_char_p)
_sig(core, "kf_pending_clear", None)
_sig(core, "kf_peek_error", _i)
_sig(core, "bridge_gpu_init", _i, _i)
_sig(core, "bridge_gpu_sync", _i)
_sig(core, "bridge_gpu_get_free_memory", _i, C.POINTER(_sz), C.POINTER(_sz))
_sig(core, "bridge_gpu_malloc", _vp, _sz)
_sig(core, "bridge_gpu_free", None, _vp)
_sig(core, "bridge_transfer_fp16", _i, _vp, _vp, _sz)
_sig(core, "bridge_read_fp16", _i, _vp, _vp, _sz)
_sig(core, "bridge_transfer_int32", _i, _vp, _vp, _sz)
_sig(core, "bridge_transfer_float32", _i, _vp, _vp, _sz)
_sig(core, "bridge_read_float32", _i, _vp, _vp, _sz)
_sig(core, "bridge_gpu_memset", None, _vp, _i, _sz)
_sig(core, "bridge_fp16_to_fp32_gpu", _i, _vp, _vp, _sz)
_sig(core, "bridge_fp32_to_fp16_gpu", _i, _vp, _vp, _sz)
_sig(core, "kf_set_stream", None, _vp)
_sig(core, "kf_get_stream", _vp)
_sig(core, "ops_gemm", _i, _vp, _i, _i, _i, _f, _vp, _i, _vp, _i, _f, _vp, _i)
_sig(core, "ops_cublas_create", _vp)
_sig(core, "ops_cublas_destroy", None, _vp)
_sig(core, "ops_log_softmax", _i, _vp, _i, _i)
_sig(core, "ops_copy", _i, _vp, _vp, _i)  # (here, not only in refpath: undeclared, ctypes passes pointers as 32-bit ints)

# ---------------------------------------------------------------- nnet_*
_sig(nnet, "nnet_create", _vp, C.c_char_p, _i)
_sig(nnet, "nnet_free", None, _vp)
_sig(nnet, "nnet_parse_summary", _i, C.c_char_p, C.c_char_p, _i)
_sig(nnet, "nnet_num_layers", _i, _vp)
_sig(nnet, "nnet_layer_info", _i, _vp, _i, C.c_char_p, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i))
_sig(nnet, "nnet_num_params", _ll, _vp)
_sig(nnet, "nnet_num_param_tensors", _i, _vp)
_sig(nnet, "nnet_param_info", _i, _vp, _i, C.c_char_p, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_ll))
_sig(nnet, "nnet_set_params", _i, _vp, _vp)
_sig(nnet, "nnet_get_params", _i, _vp, _vp)
_sig(nnet, "nnet_set_bn", _i, _vp, C.c_char_p, _i, _vp, _vp, _vp, _vp, _f, _f)
_sig(nnet, "nnet_forward", _i, _vp, _vp, _i)
_sig(nnet, "nnet_forward_ivector", _i, _vp, _vp, _i, _vp, _i, _vp)
_sig(nnet, "nnet_activation", _vp, _vp, C.c_char_p, C.POINTER(_i), C.POINTER(_i))
_sig(nnet, "nnet_backward", _i, _vp, _vp)
_sig(nnet, "nnet_backward_xent", _i, _vp, _vp, _vp)
_sig(nnet, "nnet_grad_buffer", _vp, _vp)
_sig(nnet, "nnet_master_buffer", _vp, _vp)
_sig(nnet, "nnet_weight_buffer", _vp, _vp)
_sig(nnet, "nnet_sgd", _i, _vp, _f, _f)
_sig(nnet, "nnet_set_fp8", _i, _vp, _i)
_fp = C.POINTER(_f)
_sig(nnet, "nnet_num_components", _i, _vp)
_sig(nnet, "nnet_component_info", _i, _vp, _i, C.c_char_p, _i, _fp, _fp, _fp, C.POINTER(_i), C.POINTER(_i))
_sig(nnet, "nnet_set_component_opts", _i, _vp, C.c_char_p, _f, _f, _f)
_sig(nnet, "nnet_update", _i, _vp, _f, _f, _f, _f)
_sig(nnet, "nnet_update_stats", _i, _vp, _vp, _vp, _i, _fp, _fp)
# dynamic loss scale (kf_nnet.h nnet_set_loss_scale)
_sig(nnet, "nnet_set_loss_scale", _i, _vp, _vp)
_sig(nnet, "nnet_loss_scale_ptr", _vp, _vp)
_sig(nnet, "nnet_set_loss_scale_value", _i, _vp, _f)
_sig(nnet, "nnet_loss_scale_stats", _i, _vp, _fp, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_ll), C.POINTER(_i))
_sig(nnet, "nnet_component_orthonormal", _i, _vp, _i, _fp)
_sig(nnet, "nnet_set_component_orthonormal", _i, _vp, C.c_char_p, _f)
_sig(nnet, "nnet_orthonormal_components", _i, _vp, C.POINTER(_i), _i)
_sig(nnet, "nnet_constrain_orthonormal", _i, _vp)
_sig(nnet, "nnet_orthonormal_stats", _i, _vp, _vp, _vp, _vp, _i)
_sig(nnet, "nnet_set_natural_gradient", _i, _vp, _vp)
_sig(nnet, "nnet_natural_gradient_count", _i, _vp)
_sig(nnet, "nnet_natural_gradient_stats", _i, _vp, _vp, _vp, _vp, _i)
_sig(nnet, "nnet_natural_gradient_state", _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
_sig(nnet, "nnet_bind_grad_buffer", _i, _vp, _vp)
_sig(nnet, "nnet_backward_n", _i, _vp, _vp, _i)
_sig(nnet, "nnet_debug_tensor", _vp, _vp, C.c_char_p, _i)
_sig(nnet, "nnet_create_layout", _vp, C.c_char_p, _i)
_sig(nnet, "nnet_bind_dp", _i, _vp, _vp, _ll)
_sig(nnet, "nnet_dp_plan", _i, _vp, _ll, _i, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_ll))
_sig(nnet, "nnet_dp_debug_early", _i, _vp, _i)
_sig(nnet, "nnet_set_wgrad_stream", _i, _vp, _i)
_sig(nnet, "nnet_set_implicit_dz", _i, _vp, _i)
_sig(nnet, "nnet_set_row_subsampling", _i, _vp, _i)
_sig(nnet, "nnet_row_set", _i, _vp, C.POINTER(_i), C.POINTER(_i))
_sig(nnet, "nnet_debug_backward", _i, _vp, _i, _ll)
_sig(nnet, "nnet_debug_alloc_count", _i, _vp)
_sig(core, "kf_debug_spin", _i, _vp, _ll)
_sig(nnet, "nnet_weights_changed", _i, _vp)
# per-sequence dropout (kf_nnet.h nnet_set_dropout)
_sig(nnet, "nnet_set_sequences", _i, _vp, _vp, _i)
_sig(nnet, "nnet_dropout_layers", _i, _vp, C.POINTER(_i), _i)
_sig(nnet, "nnet_set_dropout_proportion", _i, _vp, C.c_char_p, _f)
_sig(nnet, "nnet_dropout_proportion", _i, _vp, C.c_char_p, C.POINTER(_f))
_sig(nnet, "nnet_set_dropout", _i, _vp, _i, C.c_uint64)
_sig(nnet, "nnet_set_dropout_step", _i, _vp, _ll)
_sig(nnet, "nnet_dropout_step", _ll, _vp)
_sig(nnet, "nnet_dropout_mask", _i, _vp, C.c_char_p, _vp, C.POINTER(_i), C.POINTER(_i))
# SpecAugment (kf_nnet.h nnet_set_spec_augment)
_sig(nnet, "nnet_spec_augment_layers", _i, _vp, C.POINTER(_i), _i)
_sig(nnet, "nnet_spec_augment_opts", _i, _vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i))
_sig(nnet, "nnet_set_spec_augment_opts", _i, _vp, C.c_char_p, C.c_double, C.c_double, _i)
_sig(nnet, "nnet_set_spec_augment", _i, _vp, _i, C.c_uint64)
_sig(nnet, "nnet_set_spec_augment_step", _i, _vp, _ll)
_sig(nnet, "nnet_spec_augment_step", _ll, _vp)
_sig(nnet, "nnet_spec_augment_rows", _i, _vp, C.c_char_p, _vp, C.POINTER(_i))
# training-mode BatchNorm (kf_nnet.h nnet_set_bn_train)
_sig(nnet, "nnet_set_bn_train", _i, _vp, _i)
_sig(nnet, "nnet_bn_train_layers", _i, _vp, C.POINTER(_i), _i)
_sig(nnet, "nnet_set_bn_train_sites", _i, _vp, _i)
_sig(nnet, "nnet_bn_train_sites", _i, _vp)
_sig(nnet, "nnet_set_bn_train_rows", _i, _vp, _i)
_sig(nnet, "nnet_bn_train_rows", _i, _vp)
_sig(nnet, "nnet_bn_dim", _i, _vp, C.c_char_p, _i)
_sig(nnet, "nnet_bn_batch_stats", _i, _vp, C.c_char_p, _i, _vp, _vp)
_sig(nnet, "nnet_bn_stats", _i, _vp, C.c_char_p, _i, C.POINTER(C.c_double), _vp, _vp)
_sig(nnet, "nnet_bn_zero_stats", _i, _vp)
_sig(nnet, "nnet_bn_commit", _i, _vp)
# ReLU unit statistics and self-repair (kf_nnet.h nnet_set_self_repair)
_sig(nnet, "nnet_set_self_repair", _i, _vp, _i)
_sig(nnet, "nnet_self_repair_sites", _i, _vp, C.POINTER(_i), _i)
_sig(nnet, "nnet_self_repair_opts", _i, _vp, C.c_char_p, _fp, C.POINTER(C.c_double), C.POINTER(C.c_double))
_sig(nnet, "nnet_set_self_repair_opts", _i, _vp, C.c_char_p, _f, C.c_double, C.c_double)
_sig(nnet, "nnet_relu_stats", _i, _vp, C.c_char_p, C.POINTER(C.c_double), _vp, _vp)
_sig(nnet, "nnet_relu_zero_stats", _i, _vp)
_sig(nnet, "nnet_self_repair_vector", _i, _vp, C.c_char_p, _vp)
# kf_dp.h (RCCL data parallel)
_sig(core, "kf_dp_last_error", C.c_char_p)
_sig(core, "kf_dp_unique_id", _i, C.c_char_p)
_sig(core, "kf_dp_create", _vp, _i, _i, C.c_char_p, _i)
_sig(core, "kf_dp_free", None, _vp)
_sig(core, "kf_dp_rank", _i, _vp)
_sig(core, "kf_dp_world", _i, _vp)
_sig(core, "kf_dp_allreduce_mean_async", _i, _vp, _vp, _sz)
_sig(core, "kf_dp_join", _i, _vp)
_sig(core, "kf_dp_allreduce_mean", _i, _vp, _vp, _sz)
_sig(core, "kf_dp_allreduce_sum_f64", _i, _vp, _vp, _sz)
_sig(core, "kf_dp_stats", _i, _vp, C.POINTER(_ll), C.POINTER(_ll))
_sig(core, "kf_dp_debug", _i, _vp, _i, _vp, _vp, C.c_size_t)
_sig(core, "kf_dp_plan", _i, _i, C.POINTER(_ll), C.POINTER(_ll), _ll, _ll, _i, C.POINTER(_i),
     C.POINTER(_ll), C.POINTER(_ll))
_sig(core, "kf_prof_enable", None, _i)
_sig(core, "kf_prof_reserve", _i, _i)
_sig(core, "kf_prof_collect", _i, _i, C.POINTER(_ll), C.POINTER(C.c_double), C.POINTER(C.c_double))
_sig(core, "kf_prof_reset", None)
_sig(core, "kf_prof_records", _i, _i, C.POINTER(_i), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(_i))
_sig(core, "kf_prof_collect2", _i, _i, C.POINTER(_ll), C.POINTER(C.c_double), C.POINTER(C.c_double),
     C.POINTER(C.c_double))


def _err(lib_fn):
    s = lib_fn()
    return s.decode() if s else "unknown error"


def check(rc, what="kfp16"):
    if rc != 0:
        msgs = [m for m in (core.kf_last_error(), core.kf_layers_last_error(), core.ops_last_error(),
                            core.bridge_last_error(), nnet.nnet_last_error()) if m]
        stale = core.kf_pending_log()
        if stale:   # errors other HIP calls left pending, consumed by the library's entry checks
            msgs.append(b"[" + stale + b"]")
        raise KfError(f"{what}: " + "; ".join(m.decode() for m in msgs))


def pending_log():
    """kf_pending_log(): errors earlier HIP calls left pending, consumed and logged by the
    library's entry points (kf_take_pending), or None."""
    s = core.kf_pending_log()
    return s.decode() if s else None


# ---------------------------------------------------------------- device buffers
class DeviceBuffer:
    """Owning device allocation made through bridge_gpu_malloc."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        self.ptr = core.bridge_gpu_malloc(max(self.nbytes, 16))
        if not self.ptr:
            raise KfError("bridge_gpu_malloc: " + _err(core.bridge_last_error))

    def free(self):
        if self.ptr:
            core.bridge_gpu_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def upload_fp16(arr: np.ndarray) -> DeviceBuffer:
    a = np.ascontiguousarray(arr, dtype=np.float16)
    buf = DeviceBuffer(a.nbytes)
    check(core.bridge_transfer_fp16(buf.ptr, a.ctypes.data, a.size), "upload_fp16")
    buf.shape = a.shape
    return buf


def upload_f32(arr: np.ndarray) -> DeviceBuffer:
    a = np.ascontiguousarray(arr, dtype=np.float32)
    buf = DeviceBuffer(a.nbytes)
    check(core.bridge_transfer_float32(buf.ptr, a.ctypes.data, a.size), "upload_f32")
    buf.shape = a.shape
    return buf


def read_fp16(ptr, shape) -> np.ndarray:
    out = np.empty(shape, dtype=np.float16)
    check(core.bridge_read_fp16(out.ctypes.data, ptr, out.size), "read_fp16")
    return out


def read_f32(ptr, shape) -> np.ndarray:
    out = np.empty(shape, dtype=np.float32)
    check(core.bridge_read_float32(out.ctypes.data, ptr, out.size), "read_f32")
    return out


def hip_runtimes():
    """Paths of every HIP runtime mapped into this process (must be exactly one:
    import torch BEFORE kfp16 when both are used, so both bind torch's copy)."""
    with open("/proc/self/maps") as f:
        return sorted({l.split()[-1] for l in f if "libamdhip64" in l})


def assert_single_hip_runtime():
    libs = hip_runtimes()
    if len(libs) > 1:
        raise KfError(f"two HIP runtimes loaded {libs}: import torch before kfp16")


def prof_collect(cls: int):
    n, ms, fl = _ll(), C.c_double(), C.c_double()
    core.kf_prof_collect(cls, C.byref(n), C.byref(ms), C.byref(fl))
    return n.value, ms.value, fl.value


def prof_collect2(cls: int):
    """(launches, ms, algorithmic flops, algorithmic HBM bytes) of a kernel class"""
    n, ms, fl, by = _ll(), C.c_double(), C.c_double(), C.c_double()
    core.kf_prof_collect2(cls, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by))
    return n.value, ms.value, fl.value, by.value


def prof_records(max_n: int = 4096):
    """every kf_prof record since the last reset, in issue order: dicts of class, ms,
    flops, M, N, K and tile (BM * 10000 + BN; 0 for brackets that are not one GEMM)"""
    cls = (C.c_int * max_n)()
    ms = (C.c_float * max_n)()
    fl = (C.c_double * max_n)()
    mnkt = (C.c_int * (4 * max_n))()
    n = core.kf_prof_records(max_n, cls, ms, fl, mnkt)
    return [dict(cls=cls[i], ms=ms[i], flops=fl[i], M=mnkt[4 * i], N=mnkt[4 * i + 1], K=mnkt[4 * i + 2],
                 tile=mnkt[4 * i + 3]) for i in range(n)]


def halo_debug_last() -> dict:
    """kf_halo_debug_last: what the calling thread's last conv halo dispatch chose. kind
    'fused' (forward / input gradient) or 'wgrad', taken, and that kind's geometry"""
    v = (_i * 16)()
    core.kf_halo_debug_last(v, 16)
    if v[0] == 1:
        names = ("BM", "BN", "brow", "nch", "nbuf", "hpe", "hpos", "pad", "mtiles", "ntiles")
    elif v[0] == 2:
        names = ("BN", "waves", "stages", "npieces", "hpw", "splits", "kps")
    else:
        return dict(kind=None, taken=0)
    d = dict(kind="fused" if v[0] == 1 else "wgrad", taken=v[1])
    d.update({k: v[2 + i] for i, k in enumerate(names)})
    return d


_SPLICE_FIELDS = ("BM", "BN", "span", "edge_slots", "zero_slots", "image_rows", "npieces", "nimg", "b_stages",
                  "lds", "mtiles", "ntiles", "bkc")


def _splice_record(v) -> dict:
    d = dict(taken=v[1])
    d.update({k: v[2 + i] for i, k in enumerate(_SPLICE_FIELDS)})
    return d


def splice_once_plan(M, N, K, A, B, E) -> dict:
    """kf_splice_once_debug_plan: the single-staging kernel's plan for a product (no launch)"""
    v = (_i * 16)()
    if core.kf_splice_once_debug_plan(M, N, K, C.byref(A), C.byref(B), C.byref(E), v, 16) < 0:
        raise KfError("kf_splice_once_debug_plan: " + _err(core.kf_last_error))
    return _splice_record(v)


def splice_once_last() -> dict:
    """kf_splice_once_debug_last: what the calling thread's last kf_gemm_fused dispatch chose"""
    v = (_i * 16)()
    core.kf_splice_once_debug_last(v, 16)
    return _splice_record(v)


def set_stream(stream_handle) -> None:
    core.kf_set_stream(C.c_void_p(stream_handle) if stream_handle else None)


def sync() -> None:
    check(core.bridge_gpu_sync(), "sync")


# ---------------------------------------------------------------- network
class Network:
    """internal/nnet Network (forward.go:15-21) behind the nnet_* C-ABI."""

    def __init__(self, xconfig: str, max_frames: int, layout_only: bool = False):
        """layout_only: nnet_create_layout — no device storage, no GPU needed (layer,
        parameter and data-parallel bucket queries only)."""
        create = nnet.nnet_create_layout if layout_only else nnet.nnet_create
        self.h = create(xconfig.encode(), int(max_frames))
        if not self.h:
            raise KfError("nnet_create: " + _err(nnet.nnet_last_error))
        self.max_frames = int(max_frames)
        self.layers = []
        name = C.create_string_buffer(256)
        ty, di, do = _i(), _i(), _i()
        for i in range(nnet.nnet_num_layers(self.h)):
            nnet.nnet_layer_info(self.h, i, name, 256, C.byref(ty), C.byref(di), C.byref(do))
            self.layers.append((name.value.decode(), ty.value, di.value, do.value))
        self.num_params = nnet.nnet_num_params(self.h)
        self.params = {}
        r, c, off = _i(), _i(), _ll()
        for i in range(nnet.nnet_num_param_tensors(self.h)):
            nnet.nnet_param_info(self.h, i, name, 256, C.byref(r), C.byref(c), C.byref(off))
            self.params[name.value.decode()] = (r.value, c.value, off.value)
        self.T = 0

    def close(self):
        if getattr(self, "h", None):
            nnet.nnet_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # parameters --------------------------------------------------------
    def flat_params(self, named: dict) -> np.ndarray:
        flat = np.zeros(self.num_params, dtype=np.float32)
        for k, (r, c, off) in self.params.items():
            flat[off:off + r * c] = np.asarray(named[k], dtype=np.float32).reshape(-1)
        return flat

    def unflatten(self, flat: np.ndarray) -> dict:
        return {k: flat[off:off + r * c].reshape(r, c) for k, (r, c, off) in self.params.items()}

    def set_params(self, named: dict):
        flat = self.flat_params(named)
        check(nnet.nnet_set_params(self.h, flat.ctypes.data), "nnet_set_params")

    def get_params(self) -> dict:
        flat = np.empty(self.num_params, dtype=np.float32)
        check(nnet.nnet_get_params(self.h, flat.ctypes.data), "nnet_get_params")
        return self.unflatten(flat)

    def set_bn(self, layer, which, mean, var, gamma, beta, eps=1e-3, target_rms=None):
        """target_rms None: the layer's configured target-rms (1 unless a batchnorm-component
        sets one)."""
        target_rms = 0.0 if target_rms is None else target_rms
        arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (mean, var, gamma, beta)]
        check(nnet.nnet_set_bn(self.h, layer.encode(), which, *[a.ctypes.data for a in arrs],
                               float(eps), float(target_rms)), "nnet_set_bn")

    # compute -----------------------------------------------------------
    def forward(self, features_ptr, T: int):
        check(nnet.nnet_forward(self.h, features_ptr, int(T)), "nnet_forward")
        self.T = int(T)

    def forward_ivector(self, features_ptr, T: int, ivectors_ptr, seq_row0):
        """Forward with the ivector input: ivectors fp16 [B x dim] on the device, seq_row0
        int[B+1] frame offsets of the sequences (0 ... T)."""
        so = np.ascontiguousarray(seq_row0, dtype=np.int32)
        check(nnet.nnet_forward_ivector(self.h, features_ptr, int(T), ivectors_ptr, len(so) - 1,
                                        so.ctypes.data), "nnet_forward_ivector")
        self.T = int(T)

    def activation(self, layer: str):
        r, c = _i(), _i()
        p = nnet.nnet_activation(self.h, layer.encode(), C.byref(r), C.byref(c))
        if not p:
            raise KfError("nnet_activation: " + _err(nnet.nnet_last_error))
        return p, r.value, c.value

    def read_activation(self, layer: str) -> np.ndarray:
        p, r, c = self.activation(layer)
        return read_fp16(p, (r, c))

    def backward(self, out_grad_ptr, xent_grad_ptr=None):
        """nnet_backward; with xent_grad_ptr (the gradient Chain.xent wrote for the output-xent
        layer, in the forward's row form) nnet_backward_xent: both outputs' gradients."""
        if xent_grad_ptr is None:
            check(nnet.nnet_backward(self.h, out_grad_ptr), "nnet_backward")
        else:
            check(nnet.nnet_backward_xent(self.h, out_grad_ptr, xent_grad_ptr), "nnet_backward_xent")

    @property
    def grad_ptr(self):
        return nnet.nnet_grad_buffer(self.h)

    @property
    def master_ptr(self):
        return nnet.nnet_master_buffer(self.h)

    def relu_masks(self) -> dict:
        """Every layer's ReLU decisions (bit-packed on device) as uint8 per element."""
        out = {}
        for i, (name, ty, din, dout) in enumerate(self.layers):
            width = {6: dout, 7: dout, 9: None}.get(ty, 0)
            if width is None:
                width = self.params[name + ".BigW"][1]
            if not width:
                continue
            p = nnet.nnet_debug_tensor(self.h, b"mask", i)
            n = self.T * width
            raw = read_fp16(p, ((n + 15) // 16,)).view(np.uint8)
            out[name] = np.unpackbits(raw, bitorder="little")[:n]
        return out

    def read_grads(self) -> dict:
        return self.unflatten(read_f32(self.grad_ptr, (self.num_params,)))

    def bind_grad_buffer(self, ptr):
        check(nnet.nnet_bind_grad_buffer(self.h, ptr), "nnet_bind_grad_buffer")

    def set_fp8(self, on: bool = True):
        """MXFP8 forward GEMMs (kf_nnet.h nnet_set_fp8)"""
        check(nnet.nnet_set_fp8(self.h, int(on)), "nnet_set_fp8")

    def sgd(self, lr: float, momentum: float):
        check(nnet.nnet_sgd(self.h, float(lr), float(momentum)), "nnet_sgd")

    # Kaldi-style update (kf_nnet.h nnet_update) ----------------------------
    def components(self) -> list:
        """The update components, one per Kaldi nnet3 component: dicts of name, max_change,
        l2, lr_factor and tensors (the names of its parameter tensors, in layout order)."""
        names = list(self.params)
        name = C.create_string_buffer(256)
        mc, l2, lrf, first, cnt = _f(), _f(), _f(), _i(), _i()
        out = []
        for i in range(nnet.nnet_num_components(self.h)):
            check(nnet.nnet_component_info(self.h, i, name, 256, C.byref(mc), C.byref(l2), C.byref(lrf),
                                           C.byref(first), C.byref(cnt)), "nnet_component_info")
            out.append(dict(name=name.value.decode(), max_change=mc.value, l2=l2.value, lr_factor=lrf.value,
                            tensors=names[first.value:first.value + cnt.value]))
        return out

    def set_component_opts(self, name: str, max_change: float, l2: float = 0.0, lr_factor: float = 1.0):
        """Override a component's max-change (0: no limit), l2-regularize and learning-rate-factor."""
        check(nnet.nnet_set_component_opts(self.h, name.encode(), float(max_change), float(l2), float(lr_factor)),
              "nnet_set_component_opts")

    def update(self, lr: float, momentum: float, max_param_change: float = 2.0, l2_scale: float = 1.0):
        """One Kaldi-style update: momentum SGD with per-component max-change, L2 and
        learning-rate factors and the global max_param_change (0: no limit). l2_scale: Kaldi's
        factor on the L2 term, normally the minibatch's supervised frame count."""
        check(nnet.nnet_update(self.h, float(lr), float(momentum), float(max_param_change), float(l2_scale)),
              "nnet_update")

    def update_stats(self) -> dict:
        """The last update's max-change report (synchronises): norms n_c and scales s_c per
        component (in components() order), global_norm N and global_scale S."""
        n = nnet.nnet_num_components(self.h)
        norms, scales = np.empty(n, np.float32), np.empty(n, np.float32)
        gn, gs = _f(), _f()
        check(nnet.nnet_update_stats(self.h, norms.ctypes.data, scales.ctypes.data, n, C.byref(gn), C.byref(gs)),
              "nnet_update_stats")
        return dict(norms=norms, scales=scales, global_norm=gn.value, global_scale=gs.value)

    # Dynamic loss scale (kf_nnet.h nnet_set_loss_scale) ----------------------
    def set_loss_scale(self, on: bool = True, **opts):
        """Dynamic loss scaling of the fp16 step, kept on the device: sgd() / update()
        then check the gradient buffer for a non-finite value, skip the step and halve the scale
        on one, and unscale by 1 / scale otherwise. The objective has to multiply its derivative
        by the scale: hand loss_scale_ptr() to Chain.set_grad_scale. opts override
        kf_loss_scale_default_opts (init_scale 65536, growth 2, backoff 0.5, growth_interval
        2000, min_scale 1, max_scale 65536). on=False: the plain calls, as before."""
        if not on:
            check(nnet.nnet_set_loss_scale(self.h, None), "nnet_set_loss_scale")
            return
        o = KfLossScaleOpts()
        core.kf_loss_scale_default_opts(C.byref(o))
        for k, v in opts.items():
            if k not in dict(KfLossScaleOpts._fields_):
                raise TypeError(f"set_loss_scale: unknown option {k}")
            setattr(o, k, v)
        check(nnet.nnet_set_loss_scale(self.h, C.byref(o)), "nnet_set_loss_scale")

    def loss_scale_ptr(self):
        """The device float holding the scale (for Chain.set_grad_scale), None while off."""
        return nnet.nnet_loss_scale_ptr(self.h)

    def set_loss_scale_value(self, scale: float):
        """Set the scale (clamped to [min_scale, max_scale]): a checkpoint restore, tests."""
        check(nnet.nnet_set_loss_scale_value(self.h, float(scale)), "nnet_set_loss_scale_value")

    def loss_scale_stats(self) -> dict:
        """scale, since, steps, skipped, last_overflow of the loss scale (synchronises)."""
        s, since, steps, skipped, last = _f(), _i(), _ll(), _ll(), _i()
        check(nnet.nnet_loss_scale_stats(self.h, C.byref(s), C.byref(since), C.byref(steps), C.byref(skipped),
                                         C.byref(last)), "nnet_loss_scale_stats")
        return dict(scale=s.value, since=since.value, steps=steps.value, skipped=skipped.value,
                    last_overflow=bool(last.value))

    # Semi-orthogonal constraint (kf_nnet.h nnet_constrain_orthonormal) -------
    def component_orthonormal(self, name: str) -> float:
        """A component's orthonormal-constraint value: 0 off, > 0 a fixed scale, < 0 floating."""
        c = _f()
        for i, comp in enumerate(self.components()):
            if comp["name"] == name:
                check(nnet.nnet_component_orthonormal(self.h, i, C.byref(c)), "nnet_component_orthonormal")
                return c.value
        raise KeyError(name)

    def set_component_orthonormal(self, name: str, c: float):
        """Override a component's orthonormal-constraint value (its tensor must be one weight
        matrix [K x n] with K, n multiples of 32, 32 <= n <= K, n <= 512 unless c is 0)."""
        check(nnet.nnet_set_component_orthonormal(self.h, name.encode(), float(c)), "nnet_set_component_orthonormal")

    def orthonormal_components(self) -> list:
        """Names of the constrained components (value != 0), in components() order."""
        n = nnet.nnet_orthonormal_components(self.h, None, 0)
        idx = (_i * max(n, 1))()
        nnet.nnet_orthonormal_components(self.h, idx, n)
        comps = self.components()
        return [comps[idx[k]]["name"] for k in range(n)]

    def constrain_orthonormal(self):
        """One application of Kaldi's ConstrainOrthonormal to every constrained component
        (master and fp16 weights; the velocity is not touched)."""
        check(nnet.nnet_constrain_orthonormal(self.h), "nnet_constrain_orthonormal")

    def orthonormal_stats(self) -> dict:
        """The last constrain_orthonormal's report (synchronises), measured before its update:
        names, and per constrained component scale s, ratio and err = |W^T W - s^2 I|_F."""
        names = self.orthonormal_components()
        n = len(names)
        s, r, e = (np.empty(n, np.float32) for _ in range(3))
        check(nnet.nnet_orthonormal_stats(self.h, s.ctypes.data, r.ctypes.data, e.ctypes.data, n),
              "nnet_orthonormal_stats")
        return dict(names=names, scale=s, ratio=r, err=e)

    # Natural-gradient preconditioning (kf_nnet.h nnet_set_natural_gradient) ----
    def set_natural_gradient(self, on: bool = True, **opts):
        """Kaldi's NG-SGD on the weight gradients of the linear, output, tdnnf and prefinal
        components: backward() then leaves the preconditioned gradient for sgd() / update().
        opts override kf_ng_default_opts (rank_in 20, rank_out 80, update_period 4,
        num_samples_history 2000, alpha 4); every call with on=True starts the preconditioners
        from their default initial state. on=False: the plain gradients, as before."""
        if not on:
            check(nnet.nnet_set_natural_gradient(self.h, None), "nnet_set_natural_gradient")
            return
        o = KfNgOpts()
        core.kf_ng_default_opts(C.byref(o))
        for k, v in opts.items():
            if k not in dict(KfNgOpts._fields_):
                raise TypeError(f"set_natural_gradient: unknown option {k}")
            setattr(o, k, v)
        check(nnet.nnet_set_natural_gradient(self.h, C.byref(o)), "nnet_set_natural_gradient")

    def natural_gradient_stats(self) -> list:
        """The last backward's report (synchronises), one dict per preconditioned side of a
        component: name, side ("in" / "out"), gamma, rho, sum_d, t (all before that step's
        state update) and flag (True: a non-finite statistic left the state untouched)."""
        n = nnet.nnet_natural_gradient_count(self.h)
        comp, side = (_i * max(n, 1))(), (_i * max(n, 1))()
        rep = np.zeros((max(n, 1), NG_REPORT), np.float32)
        check(nnet.nnet_natural_gradient_stats(self.h, comp, side, rep.ctypes.data, n), "nnet_natural_gradient_stats")
        names = [c["name"] for c in self.components()]
        return [dict(name=names[comp[i]], side="out" if side[i] else "in", gamma=float(rep[i, 0]), rho=float(rep[i, 1]),
                     sum_d=float(rep[i, 2]), t=int(rep[i, 3]), flag=bool(rep[i, 4])) for i in range(n)]

    def natural_gradient_state(self) -> list:
        """The preconditioners' states (synchronises), in natural_gradient_stats() order: name,
        side, W [rank x dim] float32, d [rank] and rho (float64), t."""
        names = [c["name"] for c in self.components()]
        out = []
        for i in range(nnet.nnet_natural_gradient_count(self.h)):
            comp, side, dim, rank = _i(), _i(), _i(), _i()
            check(nnet.nnet_natural_gradient_state(self.h, i, C.byref(comp), C.byref(side), C.byref(dim), C.byref(rank),
                                                   None, None, None, None), "nnet_natural_gradient_state")
            W, d = np.empty((rank.value, dim.value), np.float32), np.empty(rank.value, np.float64)
            rho, t = C.c_double(), C.c_double()
            check(nnet.nnet_natural_gradient_state(self.h, i, None, None, None, None, W.ctypes.data, d.ctypes.data,
                                                   C.byref(rho), C.byref(t)), "nnet_natural_gradient_state")
            out.append(dict(name=names[comp.value], side="out" if side.value else "in", W=W, d=d, rho=rho.value,
                            t=int(t.value)))
        return out

    def dp_plan(self, bucket_bytes: int, max_buckets: int = 256):
        """[(after_step, begin, end)]: the gradient buckets nnet_backward exchanges
        (kf_nnet.h nnet_dp_plan), in issue order."""
        a, b, e = (_i * max_buckets)(), (_ll * max_buckets)(), (_ll * max_buckets)()
        n = nnet.nnet_dp_plan(self.h, int(bucket_bytes), max_buckets, a, b, e)
        if n < 0:
            raise KfError("nnet_dp_plan: " + _err(nnet.nnet_last_error))
        return [(a[i], b[i], e[i]) for i in range(n)]

    def weights_changed(self):
        """The fp16 weights were written through nnet_weight_buffer (kf_nnet.h)."""
        check(nnet.nnet_weights_changed(self.h), "nnet_weights_changed")

    def set_wgrad_stream(self, on: bool):
        """Weight gradients on their own stream, overlapping the input gradients (default
        on; kf_nnet.h nnet_set_wgrad_stream)."""
        check(nnet.nnet_set_wgrad_stream(self.h, int(on)), "nnet_set_wgrad_stream")

    def debug_backward(self, main_aff: int = -1, stall_cycles: int = 0):
        """Test hook of the two-stream backward (kf_nnet.h nnet_debug_backward): where the
        TDNN-F affine weight gradients run, and a spin of `stall_cycles` GPU cycles on the
        weight-gradient stream before each of its batches of work."""
        check(nnet.nnet_debug_backward(self.h, int(main_aff), int(stall_cycles)), "nnet_debug_backward")

    def debug_alloc_count(self) -> int:
        """Test hook (kf_nnet.h nnet_debug_alloc_count): the device blocks the net holds now."""
        return int(nnet.nnet_debug_alloc_count(self.h))

    def set_row_subsampling(self, stride: int):
        """Row-subsampled train step (kf_nnet.h nnet_set_row_subsampling): 3 = the layers above
        the conv stack run on the rows the chain objective's output rows 0 (mod 3) depend on;
        0 = off (full rows)."""
        check(nnet.nnet_set_row_subsampling(self.h, int(stride)), "nnet_set_row_subsampling")

    def row_set(self):
        """(tc, tc0, rows) of the last forward: tc compact rows (0: full rows), compact row c is
        source row rows[c] (3c for c < tc0, then the tail (T-1) - 3(tc-1-c))."""
        tc, tc0 = _i(), _i()
        check(nnet.nnet_row_set(self.h, C.byref(tc), C.byref(tc0)), "nnet_row_set")
        n, n0 = tc.value, tc0.value
        T = self.T
        c = np.arange(n, dtype=np.int64)
        rows = np.where(c < n0, 3 * c, (T - 1) - 3 * (n - 1 - c))
        return n, n0, rows

    def set_implicit_dz(self, on: bool):
        """TDNN-F input gradients without the stored dz: consumers read g through the ReLU
        mask (default off; kf_nnet.h nnet_set_implicit_dz)."""
        check(nnet.nnet_set_implicit_dz(self.h, int(on)), "nnet_set_implicit_dz")

    # per-sequence dropout (kf_nnet.h nnet_set_dropout) -------
    def set_sequences(self, seq_row0):
        """The sequence boundaries (int[B+1] frame offsets 0 ... T) of later forward() calls with
        that T; None: the whole input is one sequence."""
        if seq_row0 is None:
            check(nnet.nnet_set_sequences(self.h, None, 0), "nnet_set_sequences")
            return
        so = np.ascontiguousarray(seq_row0, dtype=np.int32)
        check(nnet.nnet_set_sequences(self.h, so.ctypes.data, len(so) - 1), "nnet_set_sequences")

    def dropout_layers(self) -> list:
        """Names of the layers with a dropout component (dropout-proportion >= 0)."""
        n = nnet.nnet_dropout_layers(self.h, None, 0)
        idx = (_i * max(n, 1))()
        nnet.nnet_dropout_layers(self.h, idx, n)
        return [self.layers[idx[i]][0] for i in range(n)]

    def set_dropout_proportion(self, p: float, layer: str = None):
        """Kaldi's set-dropout-proportion: 0 <= p <= 0.5 on `layer`, or on every layer with a
        component."""
        check(nnet.nnet_set_dropout_proportion(self.h, layer.encode() if layer is not None else None, float(p)),
              "nnet_set_dropout_proportion")

    def dropout_proportion(self, layer: str) -> float:
        """The layer's current proportion (-1: no component)."""
        p = _f()
        check(nnet.nnet_dropout_proportion(self.h, layer.encode(), C.byref(p)), "nnet_dropout_proportion")
        return p.value

    def set_dropout(self, on: bool, seed: int = 0):
        """Train-mode dropout on / off (default off) and the mask generator's 64-bit seed."""
        check(nnet.nnet_set_dropout(self.h, int(on), int(seed) & (2 ** 64 - 1)), "nnet_set_dropout")

    def set_dropout_step(self, step: int):
        """The step the next forward draws its masks with (replay)."""
        check(nnet.nnet_set_dropout_step(self.h, int(step)), "nnet_set_dropout_step")

    def dropout_step(self) -> int:
        return int(nnet.nnet_dropout_step(self.h))

    def dropout_mask(self, layer: str) -> np.ndarray:
        """The mask [B x dim] float32 the last forward drew for `layer` (synchronises)."""
        B, dim = _i(), _i()
        check(nnet.nnet_dropout_mask(self.h, layer.encode(), None, C.byref(B), C.byref(dim)), "nnet_dropout_mask")
        m = np.empty((B.value, dim.value), np.float32)
        check(nnet.nnet_dropout_mask(self.h, layer.encode(), m.ctypes.data, None, None), "nnet_dropout_mask")
        return m

    # SpecAugment (kf_nnet.h nnet_set_spec_augment) -----------
    def spec_augment_layers(self) -> list:
        """Names of the spec-augment layers, in the order of their ordinals."""
        n = nnet.nnet_spec_augment_layers(self.h, None, 0)
        idx = (_i * max(n, 1))()
        nnet.nnet_spec_augment_layers(self.h, idx, n)
        return [self.layers[idx[i]][0] for i in range(n)]

    def spec_augment_opts(self, layer: str):
        """(freq-max-proportion, time-zeroed-proportion, time-mask-max-frames) of `layer`."""
        f, z, m = C.c_double(), C.c_double(), _i()
        check(nnet.nnet_spec_augment_opts(self.h, layer.encode(), C.byref(f), C.byref(z), C.byref(m)),
              "nnet_spec_augment_opts")
        return f.value, z.value, m.value

    def set_spec_augment_opts(self, layer: str, f: float, z: float, m: int):
        """f in [0, 1], z in [0, 1), m >= 1: the xconfig keys' ranges."""
        check(nnet.nnet_set_spec_augment_opts(self.h, layer.encode(), float(f), float(z), int(m)),
              "nnet_set_spec_augment_opts")

    def set_spec_augment(self, on: bool, seed: int = 0):
        """Train-mode SpecAugment on / off (default off) and the mask generator's 64-bit seed."""
        check(nnet.nnet_set_spec_augment(self.h, int(on), int(seed) & (2 ** 64 - 1)), "nnet_set_spec_augment")

    def set_spec_augment_step(self, step: int):
        """The step the next forward draws its masks with (replay)."""
        check(nnet.nnet_set_spec_augment_step(self.h, int(step)), "nnet_set_spec_augment_step")

    def spec_augment_step(self) -> int:
        return int(nnet.nnet_spec_augment_step(self.h))

    def spec_augment_rows(self, layer: str) -> np.ndarray:
        """int32 [T]: per frame of the last forward -1 (zeroed) or the band start | count << 16
        of its sequence (synchronises)."""
        T = _i()
        check(nnet.nnet_spec_augment_rows(self.h, layer.encode(), None, C.byref(T)), "nnet_spec_augment_rows")
        rows = np.empty(T.value, np.int32)
        check(nnet.nnet_spec_augment_rows(self.h, layer.encode(), rows.ctypes.data, None), "nnet_spec_augment_rows")
        return rows

    # training-mode BatchNorm (kf_nnet.h nnet_set_bn_train) -----
    def set_batchnorm_train(self, on: bool):
        """Kaldi's training-mode BatchNorm on / off (default off) for the layers
        batchnorm_train_layers() names: batch statistics in the forward, the exact derivative in
        the backward, and the count / sum / sumsq accumulators. The frozen statistics are kept."""
        check(nnet.nnet_set_bn_train(self.h, int(on)), "nnet_set_bn_train")

    def set_batchnorm_train_sites(self, sites):
        """Which kinds of layer set_batchnorm_train governs: an int mask of
        BN_SITES' values, one of its names, or an iterable / comma-separated string of them:
        "tdnnf" (the default), "conv", "prefinal", "batchnorm" (the batchnorm-components), "all".
        Refused while the mode is on."""
        check(nnet.nnet_set_bn_train_sites(self.h, bn_sites_mask(sites)), "nnet_set_bn_train_sites")

    def batchnorm_train_sites(self) -> int:
        """The mask set_batchnorm_train_sites set (BN_SITES' values or-ed)."""
        return nnet.nnet_bn_train_sites(self.h)

    def set_batchnorm_train_rows(self, rows: str):
        """The rows a training-mode BatchNorm of a row-subsampled layer takes its statistics from
        (kf_nnet.h nnet_set_bn_train_rows): "all" (the default: the mode and
        set_row_subsampling(3) refuse each other) or "subsampled" (they combine; in a forward on the
        compact rows the statistics run over the rows 0 (mod 3), as Kaldi's do). Refused while both
        modes are on."""
        if rows not in BN_ROWS:
            raise KfError(f"batchnorm train rows: unknown policy {rows!r} (one of {', '.join(BN_ROWS)})")
        check(nnet.nnet_set_bn_train_rows(self.h, BN_ROWS[rows]), "nnet_set_bn_train_rows")

    def batchnorm_train_rows(self) -> str:
        """The policy set_batchnorm_train_rows set: "all" or "subsampled"."""
        v = nnet.nnet_bn_train_rows(self.h)
        return next(k for k, x in BN_ROWS.items() if x == v)

    def batchnorm_train_layers(self) -> list:
        """Names of the layers whose BatchNorm the switch governs under the current sites (the
        tdnnf-layers by default), in layer order."""
        n = nnet.nnet_bn_train_layers(self.h, None, 0)
        idx = (_i * max(n, 1))()
        nnet.nnet_bn_train_layers(self.h, idx, n)
        return [self.layers[idx[i]][0] for i in range(n)]

    def _bn_dim(self, layer: str, which: int = 0) -> int:
        d = nnet.nnet_bn_dim(self.h, layer.encode(), int(which))
        if d < 0:
            check(-1, "nnet_bn_dim")
        return d

    def batchnorm_batch_stats(self, layer: str, which: int = 0):
        """(mean, var) float32 [nnet_bn_dim] of the last train-mode forward of `layer`
        (synchronises); which = 1: a prefinal-layer's second BatchNorm."""
        d = self._bn_dim(layer, which)
        mean, var = np.empty(d, np.float32), np.empty(d, np.float32)
        check(nnet.nnet_bn_batch_stats(self.h, layer.encode(), int(which), mean.ctypes.data, var.ctypes.data),
              "nnet_bn_batch_stats")
        return mean, var

    def batchnorm_stats(self, layer: str, which: int = 0):
        """(count, sum, sumsq): the float64 accumulators of `layer` (synchronises)."""
        d = self._bn_dim(layer, which)
        cnt, s, q = C.c_double(), np.empty(d, np.float64), np.empty(d, np.float64)
        check(nnet.nnet_bn_stats(self.h, layer.encode(), int(which), C.byref(cnt), s.ctypes.data, q.ctypes.data),
              "nnet_bn_stats")
        return cnt.value, s, q

    def batchnorm_zero_stats(self):
        """Kaldi's ZeroComponentStats for the training-mode BatchNorms."""
        check(nnet.nnet_bn_zero_stats(self.h), "nnet_bn_zero_stats")

    def batchnorm_commit(self) -> int:
        """The accumulated statistics become the frozen ones of every governed layer with
        count > 0 (through nnet_set_bn; eps and target_rms kept); returns the layers committed."""
        n = nnet.nnet_bn_commit(self.h)
        if n < 0:
            check(-1, "nnet_bn_commit")
        return n

    # ReLU unit statistics and self-repair (kf_nnet.h nnet_set_self_repair) -----
    def set_self_repair(self, on: bool):
        """Kaldi's ReLU component statistics and self-repair on / off (default off) for the sites
        self_repair_sites() names: the ReLUs that training-mode BatchNorm governs. Every forward
        counts the active units, every backward pushes the pre-activation of a dead unit up and of
        a saturated one down. Accepted and without effect where no site exists."""
        check(nnet.nnet_set_self_repair(self.h, int(on)), "nnet_set_self_repair")

    def self_repair_sites(self) -> list:
        """Names of the layers whose ReLU the switch governs now, in layer order ([] while the
        switch or training-mode BatchNorm is off)."""
        n = nnet.nnet_self_repair_sites(self.h, None, 0)
        idx = (_i * max(n, 1))()
        nnet.nnet_self_repair_sites(self.h, idx, n)
        return [self.layers[idx[i]][0] for i in range(n)]

    def set_self_repair_opts(self, layer: str, scale: float = 1e-5, lower: float = 0.05, upper: float = 0.95):
        """A layer's self-repair-scale and thresholds (the xconfig keys' values until set)."""
        check(nnet.nnet_set_self_repair_opts(self.h, layer.encode(), float(scale), float(lower), float(upper)),
              "nnet_set_self_repair_opts")

    def self_repair_opts(self, layer: str) -> dict:
        """{"scale", "lower", "upper"} of a tdnnf, prefinal or conv layer."""
        k, lo, hi = _f(), C.c_double(), C.c_double()
        check(nnet.nnet_self_repair_opts(self.h, layer.encode(), C.byref(k), C.byref(lo), C.byref(hi)),
              "nnet_self_repair_opts")
        return {"scale": k.value, "lower": lo.value, "upper": hi.value}

    def relu_stats_raw(self, layer: str):
        """(count, value_sum, deriv_sum): the float64 accumulators of a site (synchronises)."""
        d = self._bn_dim(layer, 0)
        cnt, v, s = C.c_double(), np.empty(d, np.float64), np.empty(d, np.float64)
        check(nnet.nnet_relu_stats(self.h, layer.encode(), C.byref(cnt), v.ctypes.data, s.ctypes.data), "nnet_relu_stats")
        return cnt.value, v, s

    def relu_stats(self, layer: str) -> dict:
        """{"count", "value_avg", "deriv_avg"} of a site: Kaldi's <Count>, <ValueAvg> and <DerivAvg>
        (zeros while count is 0; synchronises)."""
        cnt, v, s = self.relu_stats_raw(layer)
        n = cnt if cnt > 0 else 1.0
        return {"count": cnt, "value_avg": v / n, "deriv_avg": s / n}

    def relu_zero_stats(self):
        """Kaldi's ZeroComponentStats: clears the ReLU statistics and the BatchNorm accumulators."""
        check(nnet.nnet_relu_zero_stats(self.h), "nnet_relu_zero_stats")

    def self_repair_vector(self, layer: str) -> np.ndarray:
        """The last backward's repair vector s of a site, float32 [D] (synchronises)."""
        s = np.empty(self._bn_dim(layer, 0), np.float32)
        check(nnet.nnet_self_repair_vector(self.h, layer.encode(), s.ctypes.data), "nnet_self_repair_vector")
        return s

    def dp_debug_early(self, on: bool):
        """Test hook: issue every gradient bucket before the backward runs (the
        negative control of the overlap tests)."""
        check(nnet.nnet_dp_debug_early(self.h, int(on)), "nnet_dp_debug_early")

    def bind_dp(self, comm, bucket_bytes: int):
        """Exchange the gradient over `comm` (kfp16.dp.Communicator) in buckets during
        nnet_backward; comm None unbinds."""
        check(nnet.nnet_bind_dp(self.h, comm.h if comm is not None else None, int(bucket_bytes)),
              "nnet_bind_dp")


# the sites of training-mode BatchNorm (kf_nnet.h KF_BN_SITE_*)
BN_SITES = {"tdnnf": 1, "conv": 2, "prefinal": 4, "batchnorm": 8, "all": 15}
# the row policies of training-mode BatchNorm under row subsampling (kf_nnet.h KF_BN_ROWS_*)
BN_ROWS = {"all": 0, "subsampled": 1}


def bn_sites_mask(sites) -> int:
    """An int mask, a name of BN_SITES, or several (an iterable or a comma-separated string)."""
    if isinstance(sites, (int, np.integer)) and not isinstance(sites, bool):
        return int(sites)
    names = [t.strip() for t in sites.split(",")] if isinstance(sites, str) else list(sites)
    mask = 0
    for n in names:
        if n not in BN_SITES:
            raise KfError(f"batchnorm train sites: unknown site {n!r} (one of {', '.join(BN_SITES)})")
        mask |= BN_SITES[n]
    return mask


def parse_summary(xconfig: str):
    """Host-layer xconfig resolution without touching the device."""
    n = nnet.nnet_parse_summary(xconfig.encode(), None, 0)
    if n < 0:
        raise KfError("nnet_parse_summary: " + _err(nnet.nnet_last_error))
    buf = C.create_string_buffer(n)
    nnet.nnet_parse_summary(xconfig.encode(), buf, n)
    lines = buf.value.decode().strip().splitlines()
    layers = [(a, int(b), int(c), int(d)) for a, b, c, d in (l.split() for l in lines[:-1])]
    return layers, int(lines[-1].split()[1])


def read_header_symbols(header: str):
    """Function names declared in include/<header> (for the ABI export test)."""
    import re
    text = open(os.path.join(INCDIR, header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    names = re.findall(r"\b([a-z][a-z0-9_]*)\s*\([^;{]*\)\s*;", text)
    return sorted(set(n for n in names if not n.startswith(("sizeof", "typedef"))))


# ---------------------------------------------------------------- kf_ops structs
MAXP = 9


class KfOperand(C.Structure):
    _fields_ = [("base", _vp), ("ld", _ll), ("nrows", _i), ("ncols", _i), ("kcontig", _i),
                ("nparts", _i), ("part_width", _i), ("T", _i), ("hout", _i), ("hsrc", _i),
                ("hmul", _i), ("hdiv", _i), ("tpolicy", _i), ("dt", _i * MAXP), ("dh", _i * MAXP),
                ("edge_t", _i * MAXP), ("edge_row", _i * MAXP), ("fmt", _i), ("scales", _vp),
                ("lds", _ll), ("mask", _vp), ("mask_rows", _i), ("tmul", _i), ("t0", _i)]


FMT_FP16, FMT_MXFP8 = 0, 1


class KfEpilogue(C.Structure):
    _fields_ = [("out", _vp), ("ldo", _ll), ("alpha", _f), ("beta", _f), ("bias", _vp), ("relu", _i),
                ("mask_out", _vp), ("scale", _vp), ("shift", _vp), ("resid", _vp), ("ldr", _ll),
                ("resid_alpha", _f), ("out2", _vp), ("ldo2", _ll), ("scale2", _vp), ("mask_in", _vp),
                ("out8", _vp), ("ldo8", _ll), ("scale8", _vp), ("out8_src", _i), ("edge_out", _vp),
                ("edge_r0", _i), ("edge_r1", _i), ("edge_src", _i),
                ("row_group", _i), ("row_stride", _i),
                ("drop", _vp), ("ld_drop", _ll), ("row_seg", _vp)]


def operand(base, ld, rows, cols, kcontig, nparts=1, part_width=None, T=None, hout=1, hsrc=1,
            hmul=0, hdiv=1, tpolicy=0, dt=(), dh=(), edges=(), scales=None, lds=0, mask=None, mask_rows=0):
    """scales != None makes an MXFP8 operand (base: e4m3 bytes, scales: E8M0, lds bytes/row);
    mask != None a masked fp16 operand (kf_ops.h: bit i of mask gates source element i of the
    first mask_rows source rows)"""
    o = KfOperand()
    if mask is not None:
        o.mask, o.mask_rows = mask, mask_rows
    if scales is not None:
        o.fmt, o.scales, o.lds = FMT_MXFP8, scales, lds
    o.base, o.ld, o.nrows, o.ncols, o.kcontig = base, ld, rows, cols, kcontig
    o.nparts, o.part_width = nparts, part_width if part_width is not None else cols
    o.T = T if T is not None else rows
    o.hout, o.hsrc, o.hmul, o.hdiv, o.tpolicy = hout, hsrc, hmul, hdiv, tpolicy
    for i in range(MAXP):
        o.edge_t[i] = -1
    for i, v in enumerate(dt):
        o.dt[i] = v
    for i, v in enumerate(dh):
        o.dh[i] = v
    for p, t, row in edges:
        o.edge_t[p] = t
        o.edge_row[p] = row
    return o


_sig(core, "kf_gemm_fused", _i, _i, _i, _i, C.POINTER(KfOperand), C.POINTER(KfOperand), C.POINTER(KfEpilogue))
_sig(core, "kf_gemm_wgrad", _i, _i, _i, _i, C.POINTER(KfOperand), C.POINTER(KfOperand), _vp, _ll, _vp, _i)
_sig(core, "kf_rows_sum", _i, _vp, _vp, _ll, _i, _i, _i)
_sig(core, "kf_rows_sum_mask", _i, _vp, _vp, _ll, _i, _i, _i, _vp)
_sig(core, "kf_dot2_rows", _i, _vp, _vp, _vp, _vp, _i, _i)
_sig(core, "kf_gemm_fused_edge", _i, _i, _i, _i, C.POINTER(KfOperand), C.POINTER(KfOperand), C.POINTER(KfEpilogue),
     _vp, _vp, _vp, _vp, _i)
_sig(core, "kf_scale_cols", _i, _vp, _ll, _vp, _vp, _ll, _i, _i)
_sig(core, "kf_gemm_wgrad_scaled", _i, _i, _i, _i, C.POINTER(KfOperand), C.POINTER(KfOperand), _vp, _ll, _vp, _i,
     _vp)
_sig(core, "kf_gemm_wgrad_target", _i, _i)
_sig(core, "kf_gemm_debug_kil", None, _i)
_sig(core, "kf_gemm_trace", None, _vp, _i, _i)
_sig(core, "kf_gemm_debug_splice_once", None, _i)
_sig(core, "kf_splice_once_debug_plan", _i, _i, _i, _i, C.POINTER(KfOperand), C.POINTER(KfOperand),
     C.POINTER(KfEpilogue), C.POINTER(_i), _i)
_sig(core, "kf_splice_once_debug_last", _i, C.POINTER(_i), _i)
_sig(core, "kf_halo_debug_last", _i, C.POINTER(_i), _i)
_sig(core, "kf_quant_mxfp8", _i, _vp, _ll, _i, _i, _i, _vp, _ll, _vp, _ll)
# non-MFMA layer pieces (csrc/layers.hip) and the ivector input path (csrc/ivector.hip)
_ip = C.POINTER(_i)
_sig(core, "kf_small_gemm", _i, _vp, _i, _vp, _vp, _i, _i, _i, _i)
_sig(core, "kf_bn_apply", _i, _vp, _vp, _ll, _i, _vp, _vp)
_sig(core, "kf_conv_c1_forward", _i, _i, _i, _i, _i, _i, _i, _ip, _ip, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
_sig(core, "kf_conv_c1_wgrad", _i, _i, _i, _i, _i, _i, _i, _ip, _ip, _vp, _vp, _vp, _vp)
_sig(core, "kf_sgd_flat", _i, _vp, _vp, _vp, _vp, _f, _f, _ll)
_sig(core, "kf_f32_to_f16_flat", _i, _vp, _vp, _ll)


class KfUpdSegment(C.Structure):
    _fields_ = [("begin", _ll), ("end", _ll), ("comp", _i), ("first_wg", _i)]


class KfUpdComp(C.Structure):
    _fields_ = [("max_change", _f), ("l2", _f), ("lr_factor", _f), ("first_wg", _i), ("num_wg", _i)]


UPD_CHUNK = 4096  # kf_ops.h KF_UPD_CHUNK
_sig(core, "kf_update_scratch_bytes", _ll, _ll, _i, _i)
_sig(core, "kf_update_maxchange", _i, _vp, _vp, _vp, _vp, _ll, _vp, _i, _vp, _i, _f, _f, _f, _f, _vp, _vp)


# dynamic loss scale (kf_ops.h kf_loss_scale_*, csrc/loss_scale.hip)
class KfLossScaleOpts(C.Structure):
    _fields_ = [("init_scale", _f), ("growth", _f), ("backoff", _f), ("growth_interval", _i),
                ("min_scale", _f), ("max_scale", _f)]


_sig(core, "kf_loss_scale_default_opts", None, _vp)
_sig(core, "kf_loss_scale_state_bytes", _ll)
_sig(core, "kf_loss_scale_scratch_bytes", _ll, _ll, _i)
_sig(core, "kf_loss_scale_init", _i, _vp, _vp)
_sig(core, "kf_loss_scale_set_scale", _i, _vp, _f)
_sig(core, "kf_loss_scale_check", _i, _vp, _vp, _ll, _vp, _i, _i, _vp)
_sig(core, "kf_loss_scale_read", _i, _vp, _fp, C.POINTER(_i), C.POINTER(_ll), C.POINTER(_ll), C.POINTER(_i))
_sig(core, "kf_update_maxchange_scaled", _i, _vp, _vp, _vp, _vp, _ll, _vp, _i, _vp, _i, _f, _f, _f, _f, _vp, _vp, _vp)
_sig(core, "kf_sgd_flat_scaled", _i, _vp, _vp, _vp, _vp, _f, _f, _ll, _vp)


class KfOrthoMat(C.Structure):
    _fields_ = [("offset", _ll), ("K", _i), ("n", _i), ("c", _f), ("reserved", _i)]


_sig(core, "kf_orthonormal_scratch_bytes", _ll, _vp, _i)
_sig(core, "kf_orthonormal_constrain", _i, _vp, _vp, _ll, _vp, _vp, _i, _vp, _vp)


# natural-gradient preconditioning (kf_ops.h kf_ng_*, csrc/natgrad.hip)
class KfNgOpts(C.Structure):
    _fields_ = [("rank_in", _i), ("rank_out", _i), ("update_period", _i), ("num_samples_history", _f),
                ("alpha", _f), ("epsilon", _f), ("delta", _f)]


class KfNgPre(C.Structure):
    _fields_ = [("D", _i), ("R", _i), ("w_off", _ll), ("h_off", _ll), ("s_off", _ll), ("st_off", _ll)]


class KfNgComp(C.Structure):
    _fields_ = [("dw_off", _ll), ("db_off", _ll), ("K", _i), ("N", _i), ("pre_in", _i), ("pre_out", _i)]


NG_MAX_RANK, NG_REPORT = 96, 8  # kf_ops.h KF_NG_MAX_RANK, KF_NG_REPORT


def ng_rp(R: int) -> int:
    """a rank as it is stored: padded with zero rows to a multiple of 32"""
    return (R + 31) // 32 * 32


def ng_w16_ld(D: int) -> int:
    """kf_ops.h KF_NG_W16_LD: the row pitch of a preconditioner's fp16 copy"""
    return (D + 7) // 8 * 8


def ng_stat_offsets(D: int, R: int) -> dict:
    """kf_ops.h KF_NG_STAT_*: where L and JT lie in a preconditioner's statistics, and their size"""
    Rp = ng_rp(R)
    return dict(L=32, JT=32 + Rp * Rp, floats=32 + Rp * Rp + D * Rp)


_sig(core, "kf_ng_default_opts", None, C.POINTER(KfNgOpts))
_sig(core, "kf_ng_init", _i, _vp, _vp, _i, C.POINTER(KfNgOpts), _vp, _vp, _vp)
_sig(core, "kf_ng_trx", _i, C.POINTER(KfOperand), _i, _vp)
_sig(core, "kf_ng_scales", _i, _vp, _vp, _i, C.POINTER(KfNgOpts), _vp, _vp, _vp)
_sig(core, "kf_ng_apply_scratch_bytes", _ll, _vp, _i, _vp, _i)
_sig(core, "kf_ng_apply", _i, _vp, _ll, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp)
_sig(core, "kf_ng_state_scratch_bytes", _ll, _vp, _i)
_sig(core, "kf_ng_state", _i, _vp, _vp, _i, C.POINTER(KfNgOpts), _i, _vp, _vp, _vp, _vp, _vp, _vp)
class KfDropLayer(C.Structure):
    _fields_ = [("mask", _vp), ("ld", _ll), ("dim", _i), ("ordinal", _i), ("p", _f), ("reserved", _i)]


_sig(core, "kf_dropout_masks", _i, _i, _vp, _i, C.c_uint64, _ll)
_sig(core, "kf_row_seg", _i, _vp, _vp, _i, _i, _i, _i)
_sig(core, "kf_bn_train_stats", _i, _vp, _ll, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
_sig(core, "kf_bn_train_apply", _i, _vp, _ll, _i, _i, _vp, _vp, _vp, _ll, _vp, _vp, _ll, _f, _vp, _ll)
_sig(core, "kf_bn_train_bwd_stats", _i, _vp, _ll, _vp, _ll, _i, _i, _vp, _vp, _f, _vp, _ll, _vp, _vp, _vp)
_sig(core, "kf_bn_block_stats", _i, _vp, _ll, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
_sig(core, "kf_bn_block_bwd_stats", _i, _vp, _ll, _vp, _ll, _i, _i, _i, _vp, _vp, _f, _vp, _vp)
_sig(core, "kf_bn_train_bwd_apply", _i, _vp, _ll, _vp, _ll, _i, _i, _vp, _vp, _f, _vp, _vp, _vp, _ll, _vp, _vp, _ll,
     _vp, _ll)
_sig(core, "kf_bn_train_bwd_stats_rows", _i, _vp, _ll, _vp, _ll, _i, _i, _i, _vp, _vp, _f, _vp, _ll, _vp, _vp, _vp)
_sig(core, "kf_bn_train_bwd_apply_rows", _i, _vp, _ll, _vp, _ll, _i, _i, _i, _vp, _vp, _f, _vp, _vp, _vp, _ll, _vp, _vp,
     _ll, _vp, _ll)
# ReLU statistics and self-repair (kf_ops.h)
class KfRepairSite(C.Structure):
    _fields_ = [("count", _vp), ("deriv", _vp), ("s", _vp), ("D", _i), ("scale", _f), ("lower", C.c_double),
                ("upper", C.c_double)]


_sig(core, "kf_bn_train_stats_relu", _i, _vp, _ll, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
_sig(core, "kf_bn_block_stats_relu", _i, _vp, _ll, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
_sig(core, "kf_relu_repair_vectors", _i, _vp, _vp, _i, _vp)
_sig(core, "kf_bn_train_bwd_apply_repair", _i, _vp, _ll, _vp, _ll, _i, _i, _vp, _vp, _f, _vp, _vp, _vp, _ll, _vp, _vp, _ll,
     _vp, _ll, _vp)
_sig(core, "kf_bn_train_bwd_apply_rows_repair", _i, _vp, _ll, _vp, _ll, _i, _i, _i, _vp, _vp, _f, _vp, _vp, _vp, _ll, _vp,
     _vp, _ll, _vp, _ll, _vp)
_sig(core, "kf_specaug_rows", _i, _vp, _vp, _i, _i, _i, _i, _f, _i, _i, C.c_uint, C.c_uint64, _ll)
_sig(core, "kf_specaug_apply", _i, _vp, _ll, _vp, _ll, _ll, _i, _vp)
_sig(core, "kf_gather_rows", _i, _vp, _vp, _ll, _i, _i, _i)
_sig(core, "kf_scatter_rows", _i, _vp, _vp, _ll, _i, _i, _i)
_sig(core, "kf_scatter_rows_from", _i, _vp, _vp, _ll, _i, _i, _i, _i)
_sig(core, "kf_rows_sum_list", _i, _vp, _vp, _ll, _ip, _i, _i)
_sig(core, "kf_layers_last_error", C.c_char_p)
_sig(core, "kf_combine_feature_maps", _i, _vp, _ll, _vp, _ll, _vp, _i, _vp, _ll, _i, _i, _i, _i)
_sig(core, "kf_combine_feature_maps_backward", _i, _vp, _ll, _vp, _i, _vp, _ll, _i, _i, _i)
_sig(core, "kf_im2col_small", _i, _vp, _ll, _i, _i, _i, _i, _i, _i, _ip, _ip, _vp, _i)
_sig(core, "kf_col2im_small", _i, _vp, _i, _i, _i, _i, _i, _i, _ip, _ip, _i, _vp, _ll)
_sig(core, "kf_rows_gemm", _i, _vp, _ll, _vp, _ll, _vp, _ll, _i, _i, _i)
_sig(core, "kf_rows_wgrad", _i, _vp, _ll, _vp, _ll, _vp, _ll, _i, _i, _i)
