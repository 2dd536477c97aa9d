"""The C-ABI library loads and exports every symbol include/vts.h declares (no compute calls: CPU-safe)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "visual-tactile-synthesis_amd", "libvts_hip.so")
HEADER = os.path.join(ROOT, "include", "vts.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vts_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_expected_surface():
    syms = declared_symbols()
    for must in ("vts_conv4x4", "vts_wgrad4x4", "vts_norm_stats", "vts_norm_bwd", "vts_ganloss", "vts_patch_gather",
                 "vts_patch_scatter_bwd", "vts_adam_flat", "vts_patchnce", "vts_last_error"):
        assert must in syms


def test_library_exports_every_declared_symbol():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "visual-tactile-synthesis_amd", "csrc"), "-j8"])
    lib = ctypes.CDLL(LIB)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, missing
    lib.vts_version.restype = ctypes.c_int
    assert lib.vts_version() >= 1
    lib.vts_last_error.restype = ctypes.c_char_p
    assert isinstance(lib.vts_last_error(), bytes)


def test_binding_lists_the_same_symbols():
    from vts import lib as L

    assert sorted(L.SYMBOLS) == declared_symbols()


def test_argument_errors_are_reported_not_crashed():
    """Null-pointer / bad-shape descriptors are rejected on the host before any launch."""
    from vts import lib as L

    lib = L.load()
    d = L.ConvDesc()
    rc = lib.vts_conv4x4(ctypes.byref(d), None)
    assert rc == -1 and b"null pointer" in lib.vts_last_error()
    n = L.NormDesc()
    assert lib.vts_norm_stats(ctypes.byref(n), None, None) == -1


def test_product_refuses_to_run_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from models import create_model
    from options.train_options import TrainOptions

    opt = TrainOptions(cmd_line="--model sinskitG --gpu_ids -1 --lambda_G1_lpips 0 --lambda_G2_lpips 0 "
                                "--use_vision_aided_loss False --checkpoints_dir /tmp/vts_t --name a").parse()
    with pytest.raises(RuntimeError, match="HIP path only"):
        create_model(opt)


# ---- the binding is derived from the header (vts/lib.py:parse_header): the parse, and what it yields, against the C compiler ----------
INCLUDE = os.path.dirname(HEADER)


def _cc():
    cc = shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler (cc) on PATH")
    return cc


def _loaded():
    from vts import lib as L

    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libvts_hip.so is not built")
    return L, L.load()


def _prototypes_c(protos):
    """a C file that includes the header and declares every function again, from the parsed types"""
    lines = ['#include "vts.h"']
    for name, (ret, params) in protos.items():
        lines.append("%s %s(%s);" % (ret, name, ", ".join("%s %s" % p for p in params) or "void"))
    return "\n".join(lines) + "\n"


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof of all 14 structs and offsetof of every field, as the host compiler lays out the real header, against the derived classes"""
    from vts import lib as L

    cc = _cc()
    structs = L.abi().structs
    assert len(structs) == 14 and set(structs) == set(L.STRUCTS)
    body = []
    for name, fields in structs.items():
        body.append('  printf("%%zu\\n", sizeof(%s));' % name)
        body += ['  printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for f, _, _ in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vts.h"\nint main(void) {\n%s\n  return 0;\n}\n' % "\n".join(body))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", INCLUDE, str(src), "-o", str(exe)])
    got = iter(int(v) for v in subprocess.check_output([str(exe)]).split())
    compared = 0
    for name, fields in structs.items():
        cls = L.STRUCTS[name]
        assert [f for f, _ in cls._fields_] == [f for f, _, _ in fields], name
        assert ctypes.sizeof(cls) == next(got), name
        for f, _, _ in fields:
            assert getattr(cls, f).offset == next(got), (name, f)
            compared += 1
    assert next(got, None) is None and compared == sum(len(f) for f in structs.values())


def test_prototypes_match_the_compiler(tmp_path):
    """C rejects a re-declaration with a conflicting type, so the parsed return and parameter types of every prototype are the header's"""
    from vts import lib as L

    cc = _cc()
    protos = L.abi().protos

    def compiles(protos, name):
        src = tmp_path / name
        src.write_text(_prototypes_c(protos))
        return subprocess.run([cc, "-fsyntax-only", "-Werror", "-I", INCLUDE, str(src)], capture_output=True, text=True)

    ok = compiles(protos, "protos.c")
    assert ok.returncode == 0, ok.stderr
    # negative control: the check can fail
    ret, params = protos["vts_channel_sum"]
    assert params[1] == ("int64_t", "nstride")
    bad = dict(protos, vts_channel_sum=(ret, [params[0], ("int", "nstride")] + params[2:]))
    wrong = compiles(bad, "protos_bad.c")
    assert wrong.returncode != 0 and "vts_channel_sum" in wrong.stderr, wrong.stderr


SNIPPET = """
/* a header in the style of vts.h ( with ; and ( in a comment */
#ifndef VTS_SNIPPET_H
#define VTS_SNIPPET_H
#include <stdint.h>
#define VTS_MAX_PARTS 3
#define VTS_ERR_BAD (-7)
#define VTS_UNIT 1099511627776.0 /* 2^40 */
typedef struct vts_inner {
  const float* data; /* [N] */
  int N, IH, IW;
  const int *img, *offx;
} vts_inner;
typedef struct vts_outer {
  vts_inner in0, in1;
  int64_t* slots[VTS_MAX_PARTS];
  int gstart[9];
  vts_inner level[VTS_MAX_PARTS];
} vts_outer;
const char* vts_name(void);
int vts_run(const vts_outer* d, int* fused /* out: 1 (fused); 0 otherwise */, float alpha,
            uint64_t seed, void** handle, void* stream);
int64_t vts_run_ws_floats(const vts_outer* d, int64_t HW);
#endif
"""


def test_parser_edge_cases():
    from vts import lib as L

    h = L.parse_header(SNIPPET)
    assert h.defines == {"VTS_MAX_PARTS": 3, "VTS_ERR_BAD": -7, "VTS_UNIT": float(2 ** 40)}
    assert isinstance(h.defines["VTS_ERR_BAD"], int) and isinstance(h.defines["VTS_UNIT"], float)
    assert list(h.structs) == ["vts_inner", "vts_outer"]
    assert h.structs["vts_inner"] == [("data", "const float*", None), ("N", "int", None), ("IH", "int", None), ("IW", "int", None),
                                      ("img", "const int*", None), ("offx", "const int*", None)]
    assert h.structs["vts_outer"] == [("in0", "vts_inner", None), ("in1", "vts_inner", None), ("slots", "int64_t*", 3), ("gstart", "int", 9),
                                      ("level", "vts_inner", 3)]
    assert list(h.protos) == ["vts_name", "vts_run", "vts_run_ws_floats"]
    assert h.protos["vts_name"] == ("const char*", [])
    assert h.protos["vts_run"] == ("int", [("const vts_outer*", "d"), ("int*", "fused"), ("float", "alpha"), ("uint64_t", "seed"),
                                           ("void**", "handle"), ("void*", "stream")])
    assert h.protos["vts_run_ws_floats"] == ("int64_t", [("const vts_outer*", "d"), ("int64_t", "HW")])
    classes = L.build_structs(h.structs)
    inner, outer = classes["vts_inner"], classes["vts_outer"]
    assert (inner.__name__, outer.__name__) == ("Inner", "Outer") and L.class_name("vts_norm_bwd_desc") == "NormBwdDesc"
    assert [t for _, t in outer._fields_] == [inner, inner, ctypes.c_void_p * 3, ctypes.c_int * 9, inner * 3]
    assert ctypes.sizeof(inner) == 8 + 3 * 4 + 4 + 2 * 8 and outer.slots.offset == 2 * ctypes.sizeof(inner)
    assert [L.ctype_of(t, classes) for t, _ in h.protos["vts_run"][1]] == [ctypes.POINTER(outer), ctypes.c_void_p, ctypes.c_float, ctypes.c_uint64,
                                                                            ctypes.c_void_p, ctypes.c_void_p]
    for bad in ("typedef struct vts_a { int x; } vts_b;", "static inline int vts_g(void) { return 0; }", "int vts_f(int x)", "int vts_f(int);"):
        with pytest.raises(ValueError):
            L.parse_header(bad)
    with pytest.raises(ValueError):
        L.ctype_of("double", classes)


RESTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}
BY_VALUE = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}


def test_every_symbol_is_typed_from_the_header():
    """after load(): argtypes of the parsed length and kind, restype of the parsed kind, for every name in SYMBOLS; one parse per process"""
    L, lib = _loaded()
    h = L.abi()
    assert L.abi() is h and L.load() is lib
    assert L.SYMBOLS == list(h.protos) and len(L.SYMBOLS) == len(declared_symbols())
    for name in L.SYMBOLS:
        ret, params = h.protos[name]
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        assert fn.restype is RESTYPES[ret], name
        for got, (ctype, pname) in zip(fn.argtypes, params):
            if not ctype.endswith("*"):
                assert got is BY_VALUE[ctype], (name, pname)
            elif ctype.replace("const ", "")[:-1] in L.STRUCTS:
                assert got is ctypes.POINTER(L.STRUCTS[ctype.replace("const ", "")[:-1]]), (name, pname)
            else:
                assert got is ctypes.c_void_p, (name, pname)
    assert (L.ACT_NONE, L.ACT_LRELU, L.ACT_RELU, L.ACT_TANH) == tuple(h.defines["VTS_ACT_" + k] for k in ("NONE", "LRELU", "RELU", "TANH"))
    assert (L.ERR_UNSUPPORTED, L.UNET_MAX_DOWNS, L.PATCHGAN_MAX_CONVS, L.MSD_MAX_SCALES) == tuple(
        h.defines["VTS_" + k] for k in ("ERR_UNSUPPORTED", "UNET_MAX_DOWNS", "PATCHGAN_MAX_CONVS", "MSD_MAX_SCALES"))


def test_scratch_size_entries_return_int64():
    """every *_ws_floats / *_floats / *_halfs / *_elems entry returns c_int64: a scratch size must not come back through a 32-bit int
    (vts_diffaug_op_ws_floats was declared `int` until this check was written; the header and its definition now say int64_t)"""
    L, lib = _loaded()
    sized = [s for s in L.SYMBOLS if s.endswith(("_ws_floats", "_floats", "_halfs", "_elems"))]
    assert {"vts_conv4x4_ws_floats", "vts_w3x3_wino_floats", "vts_clip_visual_weight_halfs", "vts_w3x3_bf16_elems"} <= set(sized)   # one per suffix
    narrow = [s for s in sized if getattr(lib, s).restype is not ctypes.c_int64]
    print("size entries %d, not c_int64: %s" % (len(sized), narrow))
    assert not narrow, narrow
