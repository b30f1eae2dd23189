"""CPU: the ctypes signature of every C entry point comes from include/opental_hip.h (opental_amd/_lib.py: signatures,
declare), and no call site of the package states a prototype or wraps a by-value scalar of its own."""
import ctypes
import os
import re

import pytest

from opental_amd import _lib as L
import test_abi_symbols as symbols

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_T_RETURNS = ("otal_conv_workspace_bytes", "otal_conv_prologue_bytes", "otal_conv_prologue_desc_bytes",
                  "otal_conv_deferred_end", "otal_maxpool3d_signbits_bytes", "otal_softnms_scratch_bytes",
                  "otal_detection_loss_scratch_floats", "otal_detection_loss_grad_floats")


@pytest.fixture(scope="module")
def lib():
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    return L.declare(ctypes.CDLL(build.LIB))


def test_signatures_name_every_declared_symbol():
    assert sorted(L.signatures()) == symbols.declared_symbols()


def test_known_signatures():
    sigs = L.signatures()
    vp = ctypes.c_void_p
    assert sigs["otal_adam_flat"] == (ctypes.c_int, [vp] * 4 + [ctypes.c_int64] + [ctypes.c_float] * 5
                                      + [ctypes.c_int, ctypes.c_float, ctypes.c_void_p])
    conv = sigs["otal_conv_fwd"][1]
    assert len(conv) == 13 and conv[11] is ctypes.c_size_t and conv[:2] == [vp, vp]
    assert sigs["otal_set_option"][1][0] is ctypes.c_char_p
    for name in ("otal_error_string", "otal_conv_last_kernel", "otal_layer_last_kernel"):
        assert sigs[name][0] is ctypes.c_char_p, name
    for name in SIZE_T_RETURNS:
        assert sigs[name][0] is ctypes.c_size_t, name
    assert sigs["otal_conv_prologue_desc_bytes"][1] == [] and sigs["otal_abi_version"][1] == []


def test_parser_refuses_types_it_does_not_know(tmp_path):
    def parse(text):
        path = tmp_path / "header.h"
        path.write_text(text)
        return L.signatures(str(path))
    with pytest.raises(ValueError, match=r"otal_x\(double v\)"):
        parse("int otal_x(double v);")
    with pytest.raises(ValueError, match=r"otal_y\(struct S s\)"):
        parse("int otal_y(struct S s);")
    split = parse("#define OTAL_N 3\n"
                  "size_t otal_z(const float* const* x,   /* the maps */\n"
                  "              int64_t n,               // how many\n"
                  "              const char* name);\n")
    assert split == {"otal_z": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_char_p])}
    with pytest.raises(RuntimeError, match="nowhere.h"):
        L.signatures(str(tmp_path / "nowhere.h"))


def test_declared_handle_converts_by_the_header(lib):
    # host functions that launch nothing; under ctypes' default int restype the first would come back as 0
    assert lib.otal_detection_loss_grad_floats(65536, 65536, 1) == 13 * 2**32
    n = lib.otal_detection_loss_scratch_floats(1, 1)
    assert type(n) is int and n > 0
    one = ctypes.c_void_p(16)  # never dereferenced: argument checks come first
    f = ctypes.cast(one, ctypes.POINTER(ctypes.c_float))
    with pytest.raises(ctypes.ArgumentError):
        lib.otal_bmp_fwd(one, f, one, 1.5, 4, 8, 2, 1, 0, None)           # a Python float for `int B`
    symbols.test_argument_errors_do_not_launch(lib)                     # the same calls with an int come back as before


def test_call_sites_state_no_prototype():
    declared = set(L.signatures())
    bad = []
    for root, _, files in os.walk(os.path.join(REPO, "opental_amd")):
        for fn in files:
            path = os.path.join(root, fn)
            if not fn.endswith(".py") or path == os.path.join(REPO, "opental_amd", "_lib.py"):
                continue
            src = open(path).read()
            for pattern in (r"otal_\w+\.(restype|argtypes)\s*=", r"ctypes\.c_(float|int64|size_t|int)\("):
                bad += [(path, m.group(0)) for m in re.finditer(pattern, src)]
            called = re.findall(r"\.(otal_\w+)\(", src)
            tables = re.findall(r"""["'](otal_\w+)["']""", "".join(re.findall(r"(?:ENTRIES = \{|Family\()[^\n]*", src)))
            bad += [(path, name) for name in called + tables if name not in declared]
    assert not bad, bad
