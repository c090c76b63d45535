"""An `nn.Module` that owns one libf5hip handle on one device (MelSpec, Vocos, BigVGAN): built on first use, rebuilt when the
device changes, destroyed when it is dropped or the module is collected -- unless a caller still holds the handle object that
`_handle()` returned: the native handle lives as long as its last holder."""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _lib
from . import weights as W
from ._lib import _dev_f32, _ptr, _stream_ptr


class Handle(C.c_void_p):
    """A native handle that destroys itself with its last reference (passes wherever the C ABI takes the raw pointer)."""
    _destroy = None

    def __del__(self):
        try:
            if self.value and self._destroy is not None:
                self._destroy(self)
        except Exception:
            pass


class NativeModule(nn.Module):
    _prefix = ""                   # entry points: <prefix>_create / _destroy / _finalize
    _load = ""                     # the entry point that takes one named tensor
    _finalize = True               # False: the handle is ready once its tensors are loaded
    _no_cpu = "the HIP vocoder only runs on a GPU: call .to('cuda') first (there is no CPU path)"

    def __init__(self):
        super().__init__()
        self._h = None
        self._h_dev = None

    def _create(self, lib, h):
        """Fills the config and calls <prefix>_create(..., byref(h)); returns its code."""
        raise NotImplementedError

    def _tensors(self):
        """[(name, host tensor)]: the weights and the host-computed aux tables."""
        raise NotImplementedError

    def _drop_handle(self):
        self._h = None
        self._h_dev = None

    def _handle(self, dev=None):
        dev = self._anchor.device if dev is None else dev
        if dev.type != "cuda":
            raise RuntimeError(self._no_cpu)
        if self._h is not None and self._h_dev == dev:
            return self._h
        self._drop_handle()
        lib = _lib.load()
        tensors = self._tensors()
        h = Handle()
        with torch.cuda.device(dev):
            _lib.check(self._create(lib, h), self._prefix + "_create")
            h._destroy = getattr(lib, self._prefix + "_destroy")     # owned from here on, whatever happens below
            st = _stream_ptr(dev)
            for name, t in tensors:
                d = _dev_f32(t, dev)
                _lib.check(getattr(lib, self._load)(h, name.encode(), _ptr(d), _lib.shape_array(d.shape), d.dim(), st),
                           f"{self._load}({name})")
            if self._finalize:
                _lib.check(getattr(lib, self._prefix + "_finalize")(h, st), self._prefix + "_finalize")
            else:
                torch.cuda.synchronize(dev)
        self._h, self._h_dev = h, dev
        return h


class NativeVocoder(NativeModule):
    """The weights of a vocoder as a host state dict (`_sd`), uploaded when the handle is built."""

    def __init__(self, cfg: dict):
        super().__init__()
        self.cfg = dict(cfg)
        self._sd: dict[str, torch.Tensor] = {}
        self._anchor = nn.Parameter(torch.zeros(1), requires_grad=False)

    def init_synthetic(self, seed: int = 0):
        self.load_state_dict(W.synthetic_state_dict(self.param_shapes(), seed=seed))
        return self

    def state_dict(self, *a, **k):
        return dict(self._sd)

    def _set_state(self, sd, strict, what):
        """The tail of a load_state_dict (after the subclass's key filtering): strict check, host copies, handle dropped."""
        shapes = self.param_shapes()
        missing = [k for k in shapes if k not in sd]
        unexpected = [k for k in sd if k not in shapes]
        if strict and (missing or unexpected):
            raise RuntimeError(f"{what} state dict mismatch: missing {missing[:4]}, unexpected {unexpected[:4]}")
        self._sd = {k: sd[k].detach().to("cpu", torch.float32) for k in shapes if k in sd}
        self._drop_handle()
        return nn.modules.module._IncompatibleKeys(missing, unexpected)

    def _tensors(self):
        if not self._sd:
            raise RuntimeError("no vocoder weights loaded")
        return list(self._sd.items()) + list(self._aux_tables())
