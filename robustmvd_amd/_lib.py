"""ctypes binding of libmvd_hip.so: the signatures and constants are read from include/mvd.h at import.
PyTorch tensors are only used for device memory and the current stream; the library sees raw device pointers.

There is NO CPU fallback: if the library is missing or cannot be loaded the import of any op raises.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmvd_hip.so")
# `make -C robustmvd_amd/csrc exp`: the same engine + experimental kernel variants selected by MVD_K3_CFG / MVD_K4_*.
# Never loaded by the product path; tools/ and the variants test route calls through it with use_experiments_library().
EXP_LIB_PATH = os.path.join(_HERE, "lib_exp", "libmvd_hip_exp.so")

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mvd.h")

_pp = ctypes.POINTER(ctypes.c_void_p)
_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
            "double": ctypes.c_double, "mvd_stream_t": ctypes.c_void_p}


def _ctype(decl, fn, is_return=False):
    """The ctypes class of one parameter (or return) declaration of `fn`.  A type outside the header's vocabulary raises: a
    guessed type would be a wrong call into the GPU library."""
    decl = " ".join(decl.replace("*", " * ").split())
    if is_return:
        if decl == "const char *":
            return ctypes.c_char_p
    elif re.fullmatch(r"[\w ]+ \* const \*( \w+)?", decl):  # a host array of device pointers
        return _pp
    elif "*" in decl:
        return ctypes.c_void_p
    for name, ctype in _SCALARS.items():
        if re.fullmatch(name if is_return else rf"{name}( \w+)?", decl):
            return ctype
    raise RuntimeError(f"include/mvd.h: {fn}: no ctypes mapping for '{decl}'")


def parse_header(text):
    """(signatures, constants) of a C header in include/mvd.h's style: every `ret mvd_name(args);` as
    name -> (restype, argtypes), and every `#define MVD_<NAME> <integer literal>` as NAME -> value."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {name: int(value, 0) for name, value in
                 re.findall(r"^[ \t]*#[ \t]*define[ \t]+MVD_(\w+)[ \t]+(0[xX][0-9a-fA-F]+|\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    signatures = {}
    for ret, fn, args in re.findall(r"([\w \t*]+?)\b(mvd_\w+)\s*\(([^()]*)\)\s*;", text):
        args = [] if args.strip() in ("", "void") else args.split(",")
        signatures[fn] = (_ctype(ret, fn, True), [_ctype(a, fn) for a in args])
    unparsed = sorted(set(re.findall(r"\b(mvd_\w+)\s*\(", text)) - set(signatures))
    if unparsed:
        raise RuntimeError(f"include/mvd.h: {unparsed[0]}: not a plain `ret name(args);` declaration")
    return signatures, constants


if not os.path.exists(HEADER_PATH):
    raise RuntimeError(f"{HEADER_PATH} not found: the binding takes every signature and constant from it")
with open(HEADER_PATH) as _f:
    # name -> (restype, argtypes), and the header's MVD_<NAME> integers as module attributes <NAME>
    SIGNATURES, _constants = parse_header(_f.read())
globals().update(_constants)
MVD_MAX_VIEWS, MVD_CLOUD_MAX_THRESHOLDS = _constants["MAX_VIEWS"], _constants["CLOUD_MAX_THRESHOLDS"]
MVD_CLOUD_PAIR_SUMS_PER_WORKGROUP = _constants["CLOUD_PAIR_SUMS_PER_WORKGROUP"]
MESH_RENDER_MAX_SMALL = 64  # ops.mesh_render's default threshold between the lane and the wave path (profiles/mesh_render.txt)

# built into the product library only (csrc/Makefile PRODSRCS): the experiments library has no variants of these
PRODUCT_ONLY = ("mvd_sweep_reduce_backward_workspace_bytes", "mvd_sweep_reduce_backward_f32")

_lib = None
_override = None  # set by use_experiments_library()


def _bind(path, skip=()):
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        if name in skip:
            continue
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """Loads libmvd_hip.so (once).  Raises RuntimeError with build instructions if it is absent."""
    global _lib
    if _override is not None:
        return _override
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP engine is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C robustmvd_amd/csrc`. There is no CPU fallback for this path.")
    _lib = _bind(LIB_PATH)
    return _lib


class use_experiments_library:
    """Context manager for tools/ and tests: inside it every op goes through libmvd_hip_exp.so (path overridable),
    whose kernel variants MVD_K3_CFG / MVD_K4_* select.  The product library is untouched and stays loaded."""

    def __init__(self, path=None):
        self.path = path or EXP_LIB_PATH

    def __enter__(self):
        global _override
        if not os.path.exists(self.path):
            raise RuntimeError(f"{self.path} not found: run `make -C robustmvd_amd/csrc exp`")
        self._prev = _override
        _override = _bind(self.path, skip=PRODUCT_ONLY)
        return _override

    def __exit__(self, *exc):
        global _override
        _override = self._prev
        return False


def check(rc, what):
    if rc != 0:
        msg = load().mvd_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (status {rc}): {msg}")


def stream_of(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def raw_stream(device):
    """torch's current stream of `device` (a torch.device with an index, as a tensor's) as the integer a hipStream_t argument
    takes: torch.cuda.current_stream(device).cuda_stream without the Stream object, 0.1 us against 1.8 us per launch."""
    return torch._C._cuda_getCurrentRawStream(device.index)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return ctypes.cast(arr, _pp), arr  # keep `arr` alive in the caller


def as_dtype(dtype, convert, t, name, shape=None, device=None):
    """Validates a tensor argument at the boundary (reference: asserts, planesweep_corr.py:444,473-483): a device tensor, on
    `device` and of `shape` where those are given, returned contiguous.  Another dtype than `dtype` is converted, or refused
    where `convert` is false."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{name}: tensor is on {t.device}; the HIP engine needs a cuda (ROCm) device tensor")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: on {t.device}, expected {device}")
    if t.dtype != dtype:
        if not convert:
            raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
        t = t.to(dtype)
    if shape is not None and t.shape != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.contiguous()


def as_f32(t, name, shape=None, device=None):
    """as_dtype for the fp32 entry points: any other dtype is converted silently."""
    return as_dtype(torch.float32, True, t, name, shape, device)


def as_f16(t, name, shape=None, device=None):
    """as_dtype for the fp16 entry points: no silent conversion, the caller decides where the rounding happens."""
    return as_dtype(torch.float16, False, t, name, shape, device)
