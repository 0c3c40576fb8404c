"""What the classes that own a handle of the C ABI share: the lifecycle of the handle (:class:`NativeHandle`), the params-layout
check, the reset mask, which batch and which segments a fly means, and the zero-copy views of device memory."""

from __future__ import annotations

import ctypes

import numpy as np

from . import _native


class NativeHandle:
    """Owner of one handle of the library.  A subclass names the entry point that destroys it, the noun of ``the ... is closed``,
    the attribute that holds it and the attributes that are views of its memory; it creates the handle with :meth:`_create`."""

    _destroy_entry = ""
    _noun = ""
    _handle_attr = "_h"
    _views = ()
    _lib = staticmethod(_native.lib)
    _creation_error = _native.NativeError                # what a refused creation raises, from the library's message

    def _create(self, entry: str, *args):
        lib = self._lib()
        handle = getattr(lib, entry)(*args)
        if not handle:
            raise self._creation_error(lib.nmf_last_error().decode())
        setattr(self, self._handle_attr, handle)
        return handle

    def close(self) -> None:
        handle = getattr(self, self._handle_attr, None)
        if handle:
            getattr(self._lib(), self._destroy_entry)(handle)
            setattr(self, self._handle_attr, None)
            for name in self._views:                     # (views of freed memory)
                setattr(self, name, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _handle(self):
        handle = getattr(self, self._handle_attr, None)
        if not handle:
            raise RuntimeError(f"the {self._noun} is closed")
        return handle


def check_params(struct, size_entry: str, module_file: str) -> None:
    """``struct`` (a ctypes mirror kept in ``module_file``) has the size the library's ``size_entry`` reports."""
    if ctypes.sizeof(struct) != getattr(_native.lib(), size_entry)():
        raise _native.NativeError(f"{size_entry[:-len('_size')]} layout mismatch between {module_file} and libnmf_hip.so")


def reset_mask(mask, n: int, sim):
    """``mask`` (``(n,)``, numpy or torch, any dtype; nonzero = set) as a contiguous uint8 tensor on ``sim``'s device; None stays."""
    if mask is None:
        return None
    t = sim._torch
    m = t.as_tensor(mask, device=sim.device)
    if tuple(m.shape) != (n,):
        raise ValueError(f"Expected a reset mask of shape ({n},), but got {tuple(m.shape)}")
    return (m != 0).to(t.uint8).contiguous()


def fly_batch(sim, fly_name: str, *, resolve: bool):
    """The batch that steps ``fly_name``: ``sim`` itself, or for a world with several flies ``sim.for_fly(fly_name)`` — which a
    class that does not ``resolve`` asks its caller to pass."""
    if hasattr(sim, "for_fly"):
        if not resolve:
            raise ValueError(f"a world with several flies has one batch per fly: pass sim.for_fly({fly_name!r})")
        sim = sim.for_fly(fly_name)
    return sim


def leg_segments(fly, legs):
    """``(root_seg, tip_seg)`` in the fly's segment order: the root segment and, int32 per leg of ``legs``, its last tarsal segment."""
    segs = [s.name for s in fly.get_bodysegs_order()]
    return segs.index(fly.root_segment.name), np.array([segs.index(f"{leg}_tarsus5") for leg in legs], dtype=np.int32)


def site_arrays(fly, sites):
    """``(seg (k,) int32, rel (k, 3) float32)`` of ``sites``, a list of (segment name, offset in the segment frame)."""
    segs = [s.name for s in fly.get_bodysegs_order()]
    return np.array([segs.index(n) for n, _ in sites], dtype=np.int32), np.array([r for _, r in sites], dtype=np.float32)


def _tensor_from_ptr(torch, ptr: int, shape, device, typestr: str = "<f4"):
    """Wrap a raw device pointer as a torch tensor without copying."""
    n = int(np.prod(shape))

    class _Holder:
        pass

    h = _Holder()
    h.__cuda_array_interface__ = {
        "shape": (max(n, 1),), "typestr": typestr, "data": (int(ptr), False), "version": 3, "strides": None,
    }
    t = torch.as_tensor(h, device=device)
    return t[:n].reshape(shape)


def _field_view(sim, field_ptr, handle, which: int, typestr: str = "<f4", shape=None):
    """Zero-copy view of field ``which`` of a native handle on ``sim``'s device, ``(n_worlds, width)`` unless ``shape`` says
    otherwise; ``field_ptr`` is the handle's ``nmf_*_field_ptr`` entry point."""
    width = ctypes.c_int32(0)
    ptr = field_ptr(handle, which, ctypes.byref(width))
    if not ptr:
        raise _native.NativeError(_native.lib().nmf_last_error().decode())
    return _tensor_from_ptr(sim._torch, ptr, shape or (sim.n_worlds, max(width.value, 0)), sim.device, typestr)
