"""ctypes binding of libdetectorch_optim_hip.so (C ABI: include/detectorch_optim_hip.h): gradient clipping by the global norm
fused with momentum SGD.

A fifth library next to libdetectorch_hip.so (hip.py), libdetectorch_train_hip.so (hip_train.py), libdetectorch_loss_hip.so
(hip_loss.py) and libdetectorch_grad_hip.so (hip_grad.py), built by build.build_optim() on first use.  PyTorch is used for device
memory and the current HIP stream only; there is NO CPU fallback: CPU tensors raise.
"""
import ctypes as C
import os

import torch

from . import build as _build
from . import hip
from .hip import _require_cuda

LIB_PATH = os.environ.get("DETECTORCH_OPTIM_HIP_LIB") or _build.OPTIM_LIB

MAX_TENSORS, MAX_ELEMENTS, MAX_TOTAL, MAX_GROUPS, CHUNK, BODY_CHUNKS = 16384, 1 << 30, 1 << 34, 64, 4096, 2048
SKIP_NONFINITE = 1


class SgdTensor(C.Structure):
    """struct dtc_sgd_tensor (include/detectorch_optim_hip.h)"""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("buf", C.c_void_p), ("n", C.c_int64), ("group", C.c_int32), ("_pad", C.c_int32)]


# include/detectorch_optim_hip.h, one row per exported function (the format of hip._SIGNATURES)
SIGNATURES = hip.signatures("""
str dtc_optim_target_arch()
size dtc_sgd_plan_bytes(n_tensors:i counts)
status dtc_sgd_plan(records:SgdTensor n_tensors:i n_groups:i plan_out plan_bytes:z n_chunks)
size dtc_sgd_workspace_bytes(n_chunks:i)
status dtc_sgd_step(plan_dev plan_bytes:z n_tensors:i n_chunks:i group_hyper_dev n_groups:i momentum:f max_norm:f flags:i workspace
    workspace_bytes:z stats stream)
""", {"SgdTensor": SgdTensor})

_lib = None


def lib():
    """Build (when stale or missing) and load the optimizer library, or fail loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if "DETECTORCH_OPTIM_HIP_LIB" not in os.environ:
        _build.build_optim()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("detectorch_amd: %s is missing. Build it with `python -m detectorch_amd.build` (hipcc, gfx950). "
                           "There is no CPU/PyTorch fallback for the clipped SGD step." % LIB_PATH)
    _lib = hip.typed(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


class Plan:
    """The device table of one set of (p, g, buf) arrays with what dtc_sgd_step needs next to it: table (uint8 on the device),
    n_tensors, n_chunks, n_groups, workspace."""

    def __init__(self, table, n_tensors, n_chunks, n_groups, workspace):
        self.table, self.n_tensors, self.n_chunks, self.n_groups, self.workspace = table, n_tensors, n_chunks, n_groups, workspace


def plan_host(records, n_groups):
    """dtc_sgd_plan over (p address, g address, buf address, n, group) rows -> (the table as a pinned uint8 host tensor, n_chunks).
    Host work only."""
    n = len(records)
    recs = (SgdTensor * max(n, 1))()
    for k, (p, g, buf, count, group) in enumerate(records):
        recs[k] = SgdTensor(p, g, buf, count, group, 0)
    counts = (C.c_int64 * max(n, 1))(*[r[3] for r in records])
    nbytes = hip.invoke(lib(), SIGNATURES, "dtc_sgd_plan_bytes", dict(n_tensors=n, counts=counts))
    host = torch.empty((max(nbytes, 16),), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    n_chunks = C.c_int(0)
    hip.invoke(lib(), SIGNATURES, "dtc_sgd_plan", dict(records=recs, n_tensors=n, n_groups=n_groups, plan_out=host.data_ptr(),
                                                       plan_bytes=nbytes, n_chunks=C.byref(n_chunks)))
    return host[:32 * n + 16 * n_chunks.value], n_chunks.value


def make_plan(params, grads, bufs, groups, n_groups):
    """The Plan of dense float32 device tensors params / grads / bufs (equal sizes per row; only 4-byte alignment is needed) with
    their group indices.  The table goes up on the current stream from a pinned buffer of its own, into device memory of its own:
    a table that a kernel in flight still reads is never overwritten.  No host sync."""
    dev = _require_cuda(*params, *grads, *bufs)
    for p, g, b in zip(params, grads, bufs):
        for t in (p, g, b):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
                raise TypeError("clipped SGD: parameters, gradients and momentum buffers must be dense contiguous float32 tensors of "
                                "equal size, got %s %s" % (t.dtype, tuple(t.shape)))
    host, n_chunks = plan_host([(p.data_ptr(), g.data_ptr(), b.data_ptr(), p.numel(), k)
                                for p, g, b, k in zip(params, grads, bufs, groups)], n_groups)
    need = hip.invoke(lib(), SIGNATURES, "dtc_sgd_workspace_bytes", dict(n_chunks=n_chunks))
    return Plan(host.to(dev, non_blocking=True), len(params), n_chunks, n_groups, hip.workspace(need, dev))


def sgd_step(plan, hyper, momentum, max_norm, stats, skip_nonfinite=False):
    """dtc_sgd_step on a Plan: hyper float32 [n_groups, 2] = (lr, wd) and stats float32 [4] on the plan's device.  One call for all
    tensors: p and buf are updated in place, g is only read, stats = (total_norm, coef, nonfinite, 0).  No host sync."""
    dev = _require_cuda(plan.table, hyper, stats)
    if hyper.dtype != torch.float32 or tuple(hyper.shape) != (plan.n_groups, 2) or not hyper.is_contiguous():
        raise TypeError("sgd_step: hyper must be a contiguous float32 [%d, 2] tensor" % plan.n_groups)
    if stats.dtype != torch.float32 or stats.numel() != 4 or not stats.is_contiguous():
        raise TypeError("sgd_step: stats must be a contiguous float32 [4] tensor")
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_sgd_step", dict(
            plan_dev=plan.table, plan_bytes=plan.table.numel(), n_tensors=plan.n_tensors, n_chunks=plan.n_chunks,
            group_hyper_dev=hyper, n_groups=plan.n_groups, momentum=momentum, max_norm=max_norm,
            flags=SKIP_NONFINITE if skip_nonfinite else 0, workspace=plan.workspace, workspace_bytes=plan.workspace.numel(),
            stats=stats))
    return stats
