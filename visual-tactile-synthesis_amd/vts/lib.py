"""ctypes binding of libvts_hip.so, derived from include/vts.h -- the only way the product path computes.

The header is the single statement of the ABI.  It is parsed once per process, when this module is imported (`abi()`, memoised), and
everything below comes out of that parse: one `ctypes.Structure` per `typedef struct vts_x` (vts_norm_bwd_desc -> NormBwdDesc, fields in
the header's order), `argtypes` / `restype` of every prototype (set by the first `load()`), `SYMBOLS`, and one module constant per
`#define VTS_NAME <number>` (VTS_ACT_LRELU -> ACT_LRELU).  A new entry point is declared in the header and wrapped in ops.py; nothing is
added here.  Type mapping: int / float / int64_t / uint64_t by value; a pointer to a vts_* struct is POINTER(Structure) (call sites pass
`byref(desc)` or a host array of descriptors); every other pointer is c_void_p, which takes `tensor.data_ptr()`, None, `byref(c_int)` and
host arrays alike.

There is deliberately NO fallback: if the shared library or the header is missing or a call fails, this module raises.  Tensors are
passed as raw device pointers (`tensor.data_ptr()`), shapes as ints, and every launch goes to torch's current HIP stream, so torch
provides memory and stream plumbing only.
"""
import collections
import ctypes as C
import functools
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VTS_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "libvts_hip.so")   # (VTS_LIB_PATH: A/B of builds, tools/)
if os.environ.get("VTS_LIB_PATH"):
    import sys
    print("NOTE: VTS_LIB_PATH overrides the in-tree library: loading %s" % LIB_PATH, file=sys.stderr, flush=True)
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "vts.h")

GAN_MODES = {"nonsaturating": 0, "lsgan": 1, "vanilla": 2, "wgan": 3, "wgangp": 3, "hinge": 4, "vanilla_sigmoid": 5}

# ---- the header, parsed: plain data, C types as normalised strings ("const float*", "vts_operand", "int64_t") -------------------------
# defines {"VTS_X": number}; structs {"vts_x": [(field, C type, array length or None)]} in the header's order;
# protos {"vts_f": (return C type, [(C type, parameter name)])} in the header's order
Header = collections.namedtuple("Header", "defines structs protos")

_DECL = re.compile(r"(.+?)([\s*]+)(\w+)\s*(?:\[\s*(\w+)\s*\])?")      # base type, stars, name, [length]
_MORE = re.compile(r"(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?")           # a further declarator of the same line: stars, name, [length]


def _declaration(text, defines):
    """`const int *img, *offx[VTS_N]` -> [("img", "const int*", None), ("offx", "const int*", N)]"""
    first, *more = [p.strip() for p in text.split(",")]
    m = _DECL.fullmatch(first)
    if not m or not all(_MORE.fullmatch(p) for p in more):
        raise ValueError("cannot parse the declaration `%s`" % " ".join(text.split()))
    base = " ".join(m.group(1).split())
    out = []
    for stars, name, length in [(m.group(2), m.group(3), m.group(4))] + [_MORE.fullmatch(p).groups() for p in more]:
        if length is not None:
            length = int(length) if length.isdigit() else defines[length]
        out.append((name, base + "*" * stars.count("*"), length))
    return out


def parse_header(text):
    """The ABI a vts.h-style header states.  Understands what that header uses and raises ValueError on anything else."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(VTS_\w+)[ \t]+\(?[ \t]*(-?[\d.]+(?:[eE][-+]?\d+)?)[ \t]*\)?[ \t]*$", text, re.M):
        defines[name] = int(value) if re.fullmatch(r"-?\d+", value) else float(value)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    structs = {}

    def struct(m):
        if m.group(1) != m.group(3):
            raise ValueError("struct %s is typedef'ed to another name, %s" % (m.group(1), m.group(3)))
        structs[m.group(1)] = [f for line in m.group(2).split(";") if line.strip() for f in _declaration(line, defines)]
        return ""

    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    protos = {}
    *chunks, tail = text.split(";")
    if tail.strip() not in ("", "}"):        # "}" closes extern "C"
        raise ValueError("cannot parse what follows the last `;`: `%s`" % " ".join(tail.split()))
    for chunk in chunks:
        if not chunk.strip():
            continue
        m = re.fullmatch(r"\s*(.+?)\s*\((.*)\)\s*", chunk, re.S)
        if not m:
            raise ValueError("cannot parse `%s`" % " ".join(chunk.split()))
        (name, ret, _), = _declaration(m.group(1), defines)
        params = [] if m.group(2).strip() == "void" else [(t, n) for p in m.group(2).split(",") for n, t, _ in _declaration(p, defines)]
        protos[name] = (ret, params)
    return Header(defines, structs, protos)


@functools.lru_cache(maxsize=None)
def abi():
    """parse_header of include/vts.h, once per process"""
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError("include/vts.h not found at %s -- the ctypes binding is derived from it.  There is no fallback table." % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


# ---- C types -> ctypes ---------------------------------------------------------------------------------------------------------------
_SCALARS = {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
_RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p}


def class_name(struct):
    """vts_norm_bwd_desc -> NormBwdDesc"""
    return "".join(w.capitalize() for w in struct[len("vts_"):].split("_"))


def ctype_of(ctype, classes):
    """the ctypes type of a parameter or field; `classes` {"vts_x": Structure}"""
    if ctype in _SCALARS:
        return _SCALARS[ctype]
    if ctype in classes:
        return classes[ctype]
    if ctype.endswith("*"):
        pointee = ctype[:-1].replace("const ", "")
        return C.POINTER(classes[pointee]) if pointee in classes else C.c_void_p
    raise ValueError("no ctypes mapping for the C type `%s`" % ctype)


def build_structs(structs):
    """{"vts_x": Structure}, built in the header's order so that a struct can hold the ones declared above it"""
    classes = {}
    for name, fields in structs.items():
        ctypes_fields = [(f, ctype_of(t, classes) if n is None else ctype_of(t, classes) * n) for f, t, n in fields]
        classes[name] = type(class_name(name), (C.Structure,), {"_fields_": ctypes_fields, "__doc__": "%s (include/vts.h)" % name})
    return classes


STRUCTS = build_structs(abi().structs)
globals().update({cls.__name__: cls for cls in STRUCTS.values()})                    # Operand, ConvDesc, WgradDesc, ReduceJob, ...
globals().update({name[len("VTS_"):]: value for name, value in abi().defines.items()})   # ACT_NONE .. ACT_TANH, ERR_UNSUPPORTED, LOSS_SCALE, ...
SYMBOLS = list(abi().protos)          # every symbol include/vts.h declares (tests/test_abi.py checks the export list against the header)

_lib = None


def load():
    """Load libvts_hip.so (once) and type every entry point from the header.  Raises if it is not built: the product has no CPU/eager path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libvts_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C visual-tactile-synthesis_amd/csrc`.  There is no fallback path." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (ret, params) in abi().protos.items():
        fn = getattr(lib, name)
        fn.argtypes = [ctype_of(t, STRUCTS) for t, _ in params]
        fn.restype = _RETURNS[ret]
    _lib = lib
    return lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, load().vts_last_error().decode()))


def ptr(t):
    return None if t is None else t.data_ptr()


def operand(t, scale=None, shift=None, C_=None, nstride=None):
    """Operand view of a contiguous NCHW tensor (or a channel slice given C_/nstride)."""
    if t is None:
        return Operand(None, None, None, 0, 0)
    assert t.dtype == torch.float32 and t.is_cuda
    c = t.shape[1] if C_ is None else C_
    ns = t.stride(0) if nstride is None else nstride
    return Operand(t.data_ptr(), ptr(scale), ptr(shift), c, ns)
