"""ctypes binding of libcseg_host.so, the native host-side helper (csrc_host/rng_draws.cpp): batched replicas of the
`torch.randperm` calls of the reference on PyTorch's default CPU generator. Optional: when the library has not been
built the callers fall back to calling `torch.randperm` once per draw -- the same stream, only slower."""
import ctypes
import os

import numpy as np
import torch  # noqa: F401  (libtorch must be loaded before the helper)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libcseg_host.so")
_lib = None
_tried = False


def lib():
    global _lib, _tried
    if not _tried:
        _tried = True
        if os.path.exists(LIB_PATH) and not os.environ.get("CSEG_NO_HOST_LIB"):
            try:
                h = ctypes.CDLL(LIB_PATH)
                h.cseg_host_randperm_prefixes.restype = ctypes.c_int
                h.cseg_host_randperm_prefixes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                          ctypes.c_void_p]
                for name in ("cseg_host_mt_export", "cseg_host_mt_import"):
                    getattr(h, name).restype = ctypes.c_int
                    getattr(h, name).argtypes = [ctypes.c_void_p]
                _lib = h
            except (OSError, AttributeError):
                _lib = None
    return _lib


def randperm_prefixes(n_list, keep, flat=False):
    """For every i: the first keep[i] entries of torch.randperm(n_list[i]), drawn in order from the default CPU
    generator (n_list[i]-1 draws each, also when keep[i] == 0). Returns a list of int64 arrays (flat: ONE array, the prefixes
    back to back)."""
    n_list = np.ascontiguousarray(n_list, dtype=np.int64)
    keep = np.ascontiguousarray(keep, dtype=np.int64)
    h = lib()
    if h is None:
        parts = [torch.randperm(int(n)).numpy()[:int(k)] for n, k in zip(n_list, keep)]
        return (np.concatenate(parts) if parts else np.empty(0, dtype=np.int64)) if flat else parts
    out = np.empty(int(keep.sum()), dtype=np.int64)
    ok = h.cseg_host_randperm_prefixes(n_list.ctypes.data_as(ctypes.c_void_p), keep.ctypes.data_as(ctypes.c_void_p),
                                       len(n_list), out.ctypes.data_as(ctypes.c_void_p))
    if ok != 1:
        raise RuntimeError("cseg_host_randperm_prefixes failed")
    if flat:
        return out
    return np.split(out, np.cumsum(keep)[:-1]) if len(keep) else []


MT_WORDS = 625     # 624 mt19937 state words + pos, the index of the next word to temper (624 = regenerate first)


def _mt_lib(what):
    h = lib()
    if h is None:
        raise RuntimeError("%s needs libcseg_host.so (csrc_host/build.py; switched off by CSEG_NO_HOST_LIB): the state of torch's "
                           "CPU generator cannot be read or written without it, and contrast.device_sampling has no fallback" % what)
    return h


def mt_export():
    """State of torch's default CPU generator as uint32 [625] (numpy): 624 state words, then pos."""
    out = np.empty(MT_WORDS, dtype=np.uint32)
    if _mt_lib("mt_export").cseg_host_mt_export(out.ctypes.data_as(ctypes.c_void_p)) != 1:
        raise RuntimeError("cseg_host_mt_export failed")
    return out


def mt_import(words):
    """Sets torch's default CPU generator to the state `words` (uint32 [625], the layout of mt_export)."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    if words.shape != (MT_WORDS,):
        raise ValueError("mt_import: expected %d words, got %s" % (MT_WORDS, words.shape))
    if _mt_lib("mt_import").cseg_host_mt_import(words.ctypes.data_as(ctypes.c_void_p)) != 1:
        raise RuntimeError("cseg_host_mt_import failed (pos must be in [1, 624])")
