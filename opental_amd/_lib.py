"""ctypes binding of libopental_hip.so (the C ABI declared in include/opental_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or a call fails, a
RuntimeError is raised.  torch is used only for device memory and the current HIP stream.
"""
import ctypes
import operator
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OTAL_LIB_PATH") or os.path.join(_HERE, "lib", "libopental_hip.so")   # override: A/B kernel builds
ABI_VERSION = 26
F32, BF16, F16, F64 = 0, 1, 2, 3
E_UNSUPPORTED = -7      # OTAL_E_UNSUPPORTED: no kernel for this call's geometry (pair launches: issue the two launches instead)

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "opental_hip.h")    # csrc/build.py: -I<repo>/include
_BY_VALUE = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}

_lib = None


def _ctype(text, decl, is_param):
    """One parameter (`const float* const* x`, `int64_t n`) or return type of `decl` as its ctypes type: `const char*` is
    c_char_p, every other pointer c_void_p (it takes ptr(t), None, ctypes arrays and buffers, cast pointers and raw addresses
    alike), and by value only what _BY_VALUE lists -- anything else raises instead of passing as ctypes' default int."""
    words = re.findall(r"\w+|\*", text)
    if "*" in words:
        return ctypes.c_char_p if words[:3] == ["const", "char", "*"] and words.count("*") == 1 else ctypes.c_void_p
    if is_param and len(words) > 1:
        words = words[:-1]                      # the parameter's name
    if len(words) != 1 or words[0] not in _BY_VALUE:
        raise ValueError(f"{decl}: no ctypes mapping for '{text.strip()}'")
    return _BY_VALUE[words[0]]


def signatures(path=HEADER_PATH):
    """{name: (restype, [argtypes])} of every `ret otal_name(params);` the header declares."""
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: the ctypes signatures are read from the C header")
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    text = re.sub(r"//[^\n]*|^[ \t]*#[^\n]*", " ", text, flags=re.M)
    sigs = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(otal_\w+)\s*\(([^()]*)\)\s*;", text):
        decl = " ".join(f"{ret} {name}({params})".split())
        params = [] if params.strip() == "void" else params.split(",")
        sigs[name] = (_ctype(ret, decl, False), [_ctype(p, decl, True) for p in params])
    return sigs


class _Int:
    """The argtypes entry of an `int` parameter.  c_int.from_param builds an argument object per call (~75 ns each, and the
    launch wrappers pass plain ints by the dozen); operator.index hands the int itself on (~10 ns), which ctypes passes as a
    C int as it always has -- and it refuses a float or None just the same (ctypes.ArgumentError)."""
    from_param = operator.index


def declare(cdll):
    """Set restype and argtypes of every entry point the header declares on a ctypes handle of the library.  This is the only
    place a prototype is stated on the Python side: call sites pass plain Python numbers and pointers."""
    for name, (restype, argtypes) in signatures().items():
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = restype, [_Int if t is ctypes.c_int else t for t in argtypes]
    return cdll


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -m opental_amd.csrc.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        if L.otal_abi_version() != ABI_VERSION:
            raise RuntimeError("libopental_hip.so ABI version mismatch; rebuild")
        declare(L)
        _lib = L
    return _lib


def set_option(name, value):
    """Run-time kernel-selection switch (include/opental_hip.h: otal_set_option); the C side reads the environment
    variable of the same name only once, at the switch's first use."""
    check(lib().otal_set_option(name.encode(), int(value)), "otal_set_option")


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: [{rc}] {lib().otal_error_string(rc).decode()}")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


STREAM_OVERRIDE = None      # a raw stream handle: launches go there instead of torch's current stream (ops.issue_on)


def stream():
    """The raw HIP stream torch is currently launching on (side streams and graph capture included).  Goes through the
    C bindings directly: torch.cuda.current_stream() builds a Stream object (~10 us) and this runs ~110 times per step."""
    if STREAM_OVERRIDE is not None:
        return ctypes.c_void_p(STREAM_OVERRIDE)
    try:
        return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))
    except AttributeError:          # private bindings moved: the public (slower) route
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dtype_code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float16:
        return F16
    if t.dtype == torch.float64:
        return F64
    raise RuntimeError(f"unsupported dtype {t.dtype} (float32 / bfloat16 / float16 / float64)")


def require_device(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("opental_amd ops run on the GPU only (tensor is on %s)" % t.device)
        if not t.is_contiguous():
            raise RuntimeError("tensor must be contiguous")


def int_array(values):
    return (ctypes.c_int * len(values))(*values)
