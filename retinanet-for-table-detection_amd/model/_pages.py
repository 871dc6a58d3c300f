"""What the page-analysis wrappers share (header.py, components.py, structure.py; the resize and skew calls of preprocess.py, the
effect call of transform.py, the render call of utils.py): the two backends a stage runs through, the page checker and the small
array helpers.  The C side of the same entries shares csrc/rtn_page_launch.h."""
import ctypes as C

import numpy as np
import torch

from . import _rt

L = _rt.L


def i32(a):
    return np.ascontiguousarray(a, np.int32)


def i64(a):
    return np.ascontiguousarray(a, np.int64)


def ptr(a):
    """The address of a NumPy table; None for an empty one."""
    return a.ctypes.data if a.size else None


def pointers(be, arrays):
    """The C array of the buffers' addresses on backend `be` (one null entry for no buffers)."""
    return (C.c_void_p * max(len(arrays), 1))(*[be.ptr(a) for a in arrays])


def starts(sizes):
    """The exclusive scan of `sizes` -> (the int64 first offsets, the total)."""
    ends = np.cumsum(np.asarray(sizes, np.int64).reshape(-1), dtype=np.int64)
    first = np.zeros(len(ends), np.int64)
    first[1:] = ends[:-1]
    return first, int(ends[-1]) if len(ends) else 0


class Twins:
    """Stages through the CPU twins (rtn_*_host) over NumPy arrays."""
    device = False

    def check(self, rc):
        if rc != 0:
            raise L.RtnError(rc, L.lib.rtn_last_error(None).decode("utf-8", "replace"))

    def empty(self, n, dtype=np.uint8):
        return np.zeros(n, dtype)

    def ptr(self, a):
        return a.ctypes.data

    def host(self, a):
        return a

    def view(self, buf, off, shape):
        return buf[off:off + int(np.prod(shape))].reshape(shape)

    def clone(self, a):
        return a.copy()

    def call(self, name, args, workspace=None, extra=()):
        """<name>_host(*args, *extra): a twin takes no workspace, `workspace` is not evaluated."""
        self.check(getattr(L.lib, name + "_host")(*args, *extra))


class Device:
    """Stages through the kernels, on the current stream, over CUDA tensors."""
    device = True
    _kinds = {np.uint8: torch.uint8, np.float32: torch.float32, np.int32: torch.int32, np.uint32: torch.int32, np.uint64: torch.int64}

    def __init__(self, dev, handle=None):
        self.dev = dev
        self.h = _rt.handle() if handle is None else handle
        self.check = self.h.check

    def empty(self, n, dtype=np.uint8):
        return torch.zeros(n, dtype=self._kinds[dtype], device=self.dev)

    def ptr(self, a):
        return a.data_ptr()

    def host(self, a):
        return a.cpu().numpy()

    def view(self, buf, off, shape):
        return buf[off:off + int(np.prod(shape))].view(shape)

    def clone(self, a):
        return a.clone()

    def call(self, name, args, workspace, extra=()):
        """<name>(handle, *args, workspace, bytes) with a fresh workspace of workspace() bytes; `extra` is the twins' alone."""
        wsb = int(workspace())
        ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=self.dev)
        self.check(getattr(L.lib, name)(self.h.raw, *args, ws.data_ptr(), wsb))


def check_pages(pages, lo, hi, device=True, upload=True):
    """-> (the pages as contiguous CUDA tensors, or NumPy arrays with device=False; [(h, w, channels)]).  A page is uint8 (H,W,3) or
    (H,W) with sides lo .. hi, a tensor or a NumPy array; with upload=False the device path takes CUDA tensors only.  ValueError
    naming the page, before anything is copied or launched."""
    pages = [p if isinstance(p, torch.Tensor) else np.asarray(p) for p in pages]
    shapes = []
    for i, p in enumerate(pages):
        if device and not upload and not (isinstance(p, torch.Tensor) and p.is_cuda):
            raise ValueError("page %d: a CUDA uint8 tensor expected, got %s" % (i, type(p).__name__))
        shape = tuple(p.shape)
        if p.dtype not in (torch.uint8, np.uint8) or not (len(shape) == 2 or (len(shape) == 3 and shape[2] == 3)):
            raise ValueError("page %d: a uint8 (H,W,3) or (H,W) page expected, got %s %s" % (i, p.dtype, shape))
        if not (lo <= shape[0] <= hi and lo <= shape[1] <= hi):
            raise ValueError("page %d: sides within %d .. %d expected, got %d x %d" % (i, lo, hi, shape[0], shape[1]))
        shapes.append((shape[0], shape[1], 1 if len(shape) == 2 else 3))
    if device:
        pages = [p if isinstance(p, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(p)) for p in pages]
        return [(p if p.is_cuda else p.cuda()).contiguous() for p in pages], shapes       # a CUDA page stays on its own device
    return [np.ascontiguousarray(p.cpu().numpy() if isinstance(p, torch.Tensor) else p) for p in pages], shapes
