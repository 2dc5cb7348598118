"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/mvd.h declares (no compute call is made: there is no GPU here), and the Python binding's
signature table covers exactly those symbols."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "mvd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mvd_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_path():
    syms = declared_symbols()
    for need in ("mvd_sweep_corr_f32", "mvd_fuse_views_f32", "mvd_warp_variance_f32", "mvd_conv3d_bn_relu_f32",
                 "mvd_softmax_regress_f32", "mvd_conv2d_bn_relu_f32", "mvd_pack_conv2d_weights_f32", "mvd_bias_leaky_relu_f32",
                 "mvd_version", "mvd_last_error"):
        assert need in syms


def test_library_exports_every_declared_symbol():
    from robustmvd_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(lib, s), f"{s} declared in include/mvd.h but not exported"
    assert sorted(_lib.SIGNATURES) == declared_symbols()
    lib.mvd_version.restype = ctypes.c_int
    assert lib.mvd_version() == 100


def test_missing_library_fails_loudly(monkeypatch):
    from robustmvd_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libmvd_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load()


def test_argument_validation_without_gpu():
    import torch
    from robustmvd_amd import ops
    with pytest.raises(ValueError, match="cuda"):
        ops.softmax_regress(torch.zeros(1, 4, 2, 2), torch.zeros(1, 4))
    with pytest.raises(ValueError):
        ops.sweep_corr("nope", [], None, [], [], None)


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "robustmvd_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f"{f} imports the oracle"


def test_product_library_never_reads_the_environment():
    """include/mvd.h: "no global mutable state".  The shipped library must not import getenv and must not carry the
    experiment selectors' names; those exist only in the separate experiments build (`make exp`)."""
    import subprocess
    from robustmvd_amd import _lib
    und = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"MVD_K3_CFG", b"MVD_K4_NOMARCH", b"MVD_K4_NOKSPLIT", b"MVD_K4_DECONV_CLASSES", b"MVD_K4_MARCH_MIN",
                 b"MVD_K4_XCD", b"MVD_K4_CONV0_DZ", b"MVD_K4_MARCH_MT"):
        assert name not in blob, f"{name.decode()} is compiled into the product library"
    for f in os.listdir(os.path.join(ROOT, "robustmvd_amd", "csrc")):
        if f.endswith((".hip", ".h")) and f != "mvd_api.hip":
            assert "getenv" not in open(os.path.join(ROOT, "robustmvd_amd", "csrc", f)).read(), f


SYNTHETIC_HEADER = """
#define MVD_ANSWER 42
#define MVD_FLAG 0x10 /* hexadecimal */
#define MVD_NOT_AN_INTEGER 1.5f
typedef void* mvd_stream_t;
const char* mvd_every_type(const float* a, float* const* b, const unsigned char* const* c, void* d, int e, long long f,
                           size_t g, float h, double i, mvd_stream_t stream);
size_t mvd_two_lines(int first, /* a comment, with a comma (and brackets) */
                     const void* second);  // trailing
int mvd_no_arguments(void);
"""


def test_signatures_are_derived_from_the_header_text():
    from robustmvd_amd import _lib
    sigs, consts = _lib.parse_header(SYNTHETIC_HEADER)
    pp = ctypes.POINTER(ctypes.c_void_p)
    assert sigs == {
        "mvd_every_type": (ctypes.c_char_p, [ctypes.c_void_p, pp, pp, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong,
                                             ctypes.c_size_t, ctypes.c_float, ctypes.c_double, ctypes.c_void_p]),
        "mvd_two_lines": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_void_p]),
        "mvd_no_arguments": (ctypes.c_int, []),
    }
    assert consts == {"ANSWER": 42, "FLAG": 16}


@pytest.mark.parametrize("declaration", ["int mvd_takes_short(int n, short flag);", "short mvd_takes_short(int n);",
                                         "int mvd_takes_short(const int n);", "int mvd_takes_short(unsigned n);",
                                         "int mvd_takes_short(void (*callback)(int), int n);"])
def test_an_unmapped_type_is_refused_by_name(declaration):
    from robustmvd_amd import _lib
    with pytest.raises(RuntimeError, match="mvd_takes_short"):
        _lib.parse_header("int mvd_fine(int n);\n" + declaration)


def test_every_integer_define_of_the_header_is_exposed():
    from robustmvd_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvd.h")).read(), flags=re.S)
    defines = re.findall(r"^#define MVD_(\w+)\s+(0x[0-9a-fA-F]+|\d+)\s*$", text, flags=re.M)
    assert len(defines) >= 37
    for name, value in defines:
        assert getattr(_lib, name) == int(value, 0), name
    for name in ("MVD_MAX_VIEWS", "MVD_CLOUD_MAX_THRESHOLDS", "MVD_CLOUD_PAIR_SUMS_PER_WORKGROUP"):
        assert getattr(_lib, name) == getattr(_lib, name[4:])
    assert _lib.VERSION == 100 and _lib.MESH_RENDER_MAX_SMALL == 64
