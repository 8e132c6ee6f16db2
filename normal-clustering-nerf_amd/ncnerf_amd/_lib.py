"""ctypes binding of libncnerf.so, derived from the C ABI declared in the headers of include/ that
HEADERS lists.

This is the only place Python talks to the HIP kernels.  There is NO CPU fallback: if the library
is missing, or a kernel is called with a CPU tensor, the call raises.  Tensors are passed as raw
device pointers and sizes, on torch's *current* HIP stream (never the legacy default stream).

The headers are the single statement of the ABI, functions and constants: parsed at import in one
pass (`load_headers`) into ABI (every entry point's restype and parameters), HEADER_OF (the header a
name comes from) and CONSTANTS (every `#define NCN_<NAME> <literal>`; the Python modules look their
values up here instead of retyping them).  ABI gives every argtypes / restype, and `call` marshals
plain arguments against it (see `marshal`) before anything is launched.  A new header is one more
entry of HEADERS.
"""
import ctypes
import operator
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NCN_LIB_PATH") or os.path.join(_HERE, "libncnerf.so")  # (override: diagnostics)
INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include")
# The one place a header is named: file name -> what is derived from it (a missing file's message says
# so).  All share ncnerf.h's grammar; the order is the order of ABI and of symbols().
_DERIVED = {
    "ncnerf.h": "the binding",
    "ncnerf_metrics.h": "the binding of the validation metrics",
    "ncnerf_geom.h": "the binding of the geometry supervision",
    "ncnerf_mesh.h": "the binding of the isosurface extraction",
    "ncnerf_heads.h": "the binding of the semantic / normal heads",
    "ncnerf_sem.h": "the binding of the semantic metrics",
    "ncnerf_input_grad.h": "the binding of the split backward's direction gradient",
}
HEADERS = tuple(_DERIVED)

P = ctypes.c_void_p
I64 = ctypes.c_int64
I32 = ctypes.c_int
U32 = ctypes.c_uint32
F32 = ctypes.c_float
F64 = ctypes.c_double
U64 = ctypes.c_uint64


class NcnError(RuntimeError):
    pass


# The grammar of include/ncnerf.h (stated at its top): `ret name(type name, ...);` over these types.
_RESTYPES = {"int": ctypes.c_int, "int64_t": I64, "const char*": ctypes.c_char_p}
_SCALARS = {"int": I32, "int32_t": I32, "int64_t": I64, "uint32_t": U32, "uint64_t": U64, "float": F32, "double": F64}
_POINTEES = {"void": 0, "float": 4, "double": 8, "int": 4, "int32_t": 4, "int64_t": 8, "uint8_t": 1, "uint16_t": 2,
             "uint32_t": 4}
_DECL = re.compile(r"(const\s+char\s*\*|int64_t|int)\s*(\w+)\s*\(([^()]*)\)")
_PARAM = re.compile(r"(?:const\s+)?(\w+)(?:\s*((?:\*\s*(?:const\b\s*)?)+)|\s+)(\w+)")


def parse_header(text):
    """{name: (restype, [(kind, pointee_bytes, param_name), ...])} of every declaration of a C header
    in ncnerf.h's grammar.  restype and a scalar's kind are the C type's name; a pointer's kind is
    "ptr" and pointee_bytes the width of what it points to (0 for void, 8 for a pointer).  Anything
    outside the grammar is a ValueError naming the declaration: nothing is guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    if re.search(r"^\s*#.*\\$", text, flags=re.M):
        raise ValueError("ncnerf.h grammar: a preprocessor line is continued with a backslash")
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    text, n_extern = re.subn(r'extern\s+"C"\s*\{', "", text)
    text = text.strip()
    if n_extern == 1 and text.endswith("}"):
        text = text[:-1]
    *decls, rest = text.split(";")
    if rest.strip():
        raise ValueError(f"ncnerf.h grammar: no ';' after {' '.join(rest.split())!r}")
    out = {}
    for decl in decls:
        decl = " ".join(decl.split())
        m = _DECL.fullmatch(decl)
        if m is None:
            raise ValueError(f"ncnerf.h grammar: not `int|int64_t|const char* name(params)`: {decl!r}")
        ret, name, params = m.groups()
        if name in out:
            raise ValueError(f"ncnerf.h grammar: {name} is declared twice")
        plist = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            pm = _PARAM.fullmatch(p.strip())
            if pm is None or pm.group(3) in _POINTEES or pm.group(3) in _SCALARS or pm.group(3) == "const":
                raise ValueError(f"ncnerf.h grammar: parameter {p.strip()!r} of {decl!r} is not `type name`")
            base, stars, pname = pm.group(1), (pm.group(2) or "").count("*"), pm.group(3)
            if stars == 0 and base in _SCALARS:
                plist.append((base, 0, pname))
            elif stars == 1 and base in _POINTEES:
                plist.append(("ptr", _POINTEES[base], pname))
            elif stars == 2 and base == "void":
                plist.append(("ptr", 8, pname))
            else:
                raise ValueError(f"ncnerf.h grammar: unknown type in parameter {p.strip()!r} of {decl!r}")
        out[name] = ("const char*" if ret.startswith("const") else ret, plist)
    return out


def header_path(name, include_dir=INCLUDE_DIR):
    return os.path.join(include_dir, name)


def read_header(name, include_dir=INCLUDE_DIR):
    path = header_path(name, include_dir)
    try:
        return open(path).read()
    except OSError as e:
        raise NcnError(f"include/{name} not found at {path}: {_DERIVED[name]} is derived from it ({e})") from None


_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(NCN_\w+)(.*)$", flags=re.M)
_INT = re.compile(r"[+-]?(?:0|[1-9]\d*)")
_FLOAT = re.compile(r"[+-]?(?:(?:\d+\.\d*|\.\d+)(?:[eE][+-]?\d+)?|\d+[eE][+-]?\d+)[fF]?")


def parse_constants(text):
    """({name: int | float}, [left-out names]) of a header's `#define NCN_<NAME> <body>` lines.  A body
    that is a decimal integer or a C floating literal (an `f` suffix allowed) is a constant; any other
    (an expression, a function-like macro, a brace list) is left out by name: nothing is evaluated."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants, left_out = {}, []
    for name, body in _DEFINE.findall(text):
        body = body.strip()
        if name in constants or name in left_out:
            raise ValueError(f"ncnerf.h grammar: {name} is defined twice")
        if _INT.fullmatch(body):
            constants[name] = int(body)
        elif _FLOAT.fullmatch(body):
            constants[name] = float(body.rstrip("fF"))
        else:
            left_out.append(name)
    return constants, left_out


def load_headers(include_dir=INCLUDE_DIR):
    """(abi, header_of, constants, left_out) of every header of HEADERS under include_dir, in that order:
    abi is {entry point: (restype, params)}, header_of {entry point or define: header file name}.  A name
    that two headers declare or define is an NcnError naming both."""
    abi, header_of, constants, left_out = {}, {}, {}, []
    for header in HEADERS:
        text = read_header(header, include_dir)
        decls = parse_header(text)
        values, opaque = parse_constants(text)
        for name in (*decls, *values, *opaque):
            if name in header_of:
                raise NcnError(f"{name} is declared in include/{header} and in include/{header_of[name]}")
            header_of[name] = header
        abi.update(decls)
        constants.update(values)
        left_out += opaque
    return abi, header_of, constants, tuple(left_out)


# ABI: every entry point's (restype, parameters); HEADER_OF: the header that declares (or defines) a name;
# CONSTANTS: every `#define NCN_<NAME> <literal>`; NON_LITERAL_DEFINES: the defines that are no literal
ABI, HEADER_OF, CONSTANTS, NON_LITERAL_DEFINES = load_headers()
AMP_INIT_SCALE = CONSTANTS["NCN_AMP_INIT_SCALE"]  # torch GradScaler's init_scale


def declaration(name):
    """(restype, parameters) of an entry point, whichever header declares it."""
    return ABI[name]


def symbols(header=None):
    """The entry points of one header of HEADERS in declaration order, or of all of them in HEADERS order."""
    if header is not None and header not in HEADERS:
        raise KeyError(header)
    return [name for name in ABI if header is None or HEADER_OF[name] == header]


def exported_symbols():
    """Every name libncnerf.so must export: all headers' entry points."""
    return symbols()


# name -> argtypes (stream last), as ctypes sees them
SIGNATURES = {name: [P if kind == "ptr" else _SCALARS[kind] for kind, _, _ in params]
              for name, (_, params) in ABI.items()}

_lib = None

# Optional per-kernel timing: when TIMING is a dict, `call` brackets each launch of the entry points
# that are keys of TIMING with HIP events on the current stream (the stream the kernel runs on) and
# appends (start, end) to TIMING[name].  A GPU spin (torch.cuda._sleep) is queued in front of the
# start event so the device is still busy while Python issues the launch: the events then bracket
# the kernel itself, not the ~6 us of host-side launch latency (checked against rocprofv3).
TIMING = None
TIMING_SPIN_CYCLES = 60000


def lib():
    """Load libncnerf.so (after torch's HIP runtime, so both share one libamdhip64)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NcnError(f"libncnerf.so not found at {LIB_PATH}: run __graft_entry__.build() "
                           f"(make -C normal-clustering-nerf_amd)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (ret, _) in ABI.items():
            fn = getattr(L, name)
            fn.argtypes = SIGNATURES[name]
            fn.restype = _RESTYPES[ret]
        _lib = L
    return _lib


# ---- marshalling: one function per entry point, generated once from the header's parameters
# (straight-line code: a Python call per argument costs more than the wrappers it replaces) ----
_Tensor = torch.Tensor
_CTYPES = (ctypes.c_int.__mro__[-2], type(ctypes.byref(ctypes.c_int())))  # _CData, and what byref() returns
_AUTO = object()  # the omitted stream


def _launches(params):
    return bool(params) and params[-1] == ("ptr", 0, "stream")


def _refuse(name, i, a):
    params = declaration(name)[1]
    kind, width, pname = params[i]
    expected = f"a host {kind}" if kind != "ptr" else (
        f"a {'CUDA ' if _launches(params) else ''}tensor{' of %d-byte elements' % width if width else ''}, "
        f"None or a ctypes pointer")
    got = f"a {a.dtype} {a.device.type} tensor" if isinstance(a, _Tensor) else f"{type(a).__name__} {a!r}"
    raise TypeError(f"{name}: argument {i} ({pname}) takes {expected}, got {got}")


def _number(name, i, a, convert):
    """An int / float parameter's value that is neither an exact int / float nor a ctypes instance: never a
    device tensor into a host number (that would hide a synchronisation), and float() would parse a str."""
    if isinstance(a, (_Tensor, str, bytes, bytearray)):
        _refuse(name, i, a)
    try:
        return convert(a)
    except TypeError:
        _refuse(name, i, a)


def _marshal_source(name, params):
    launches = _launches(params)
    n = len(params)
    src = [f"def marshal({', '.join(f'a{i}' for i in range(n))}{'=_AUTO' if launches else ''}):"]
    for i, (kind, width, _) in enumerate(params):
        a = f"a{i}"
        if kind == "ptr":
            bad = ([f"{a}.element_size() != {width}"] if width else []) + ([f"not {a}.is_cuda"] if launches else [])
            auto = launches and i == n - 1
            src += [f" if {a} is _AUTO: {a} = stream()"] if auto else []
            src += [f" {'el' if auto else ''}if isinstance({a}, _Tensor):"]
            src += [f"  if {' or '.join(bad)}: _refuse({name!r}, {i}, {a})"] if bad else []
            src += [f"  {a} = {a}.data_ptr()",
                    f" elif {a} is not None and not isinstance({a}, _CTYPES): _refuse({name!r}, {i}, {a})"]
        else:
            exact, convert = ("float", "float") if kind in ("float", "double") else ("int", "operator.index")
            src += [f" if type({a}) is not {exact} and not isinstance({a}, _CTYPES):"
                    f" {a} = _number({name!r}, {i}, {a}, {convert})"]
    src += [f" return ({''.join(f'a{i}, ' for i in range(n))})"]
    return "\n".join(src)


def _marshaller(name, params):
    ns = {}
    exec(_marshal_source(name, params), globals(), ns)  # globals(): `stream` is looked up when the call is made
    n = len(params)
    return ns["marshal"], (n - 1, n) if _launches(params) else (n,)


_PLANS = {name: _marshaller(name, params) for name, (_, params) in ABI.items()}


def marshal(name, args):
    """The argument tuple `call` hands to ctypes.  Per declared parameter: a ctypes instance passes
    untouched; a pointer takes None or a tensor (of the pointee's width unless that is void; a CUDA
    tensor when the function takes a stream, i.e. launches); an integer takes operator.index(x), a
    float float(x), never a tensor.  A function whose last parameter is `void* stream` may be given
    without it: the current stream is appended, after every check.  Anything else is a TypeError."""
    fn, counts = _PLANS[name]
    if len(args) not in counts:
        decl = ", ".join(f"{'pointer' if kind == 'ptr' else kind} {pname}" for kind, _, pname in declaration(name)[1])
        raise TypeError(f"{name}: takes {' or '.join(map(str, counts))} arguments, got {len(args)}: {name}({decl})")
    return fn(*args)


def call(name, *args):
    args = marshal(name, args)
    if TIMING is not None and name in TIMING:
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(TIMING_SPIN_CYCLES)
        e0.record()
        rc = getattr(lib(), name)(*args)
        e1.record()
        TIMING[name].append((e0, e1))
    else:
        rc = getattr(lib(), name)(*args)
    if rc != 0:
        msg = lib().ncn_last_error().decode(errors="replace")
        raise NcnError(f"{name} failed (hipError {rc}): {msg}")
    return rc


def stream():
    return P(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Raw device pointer of a CUDA tensor (None -> NULL)."""
    if t is None:
        return P(None)
    return P(t.data_ptr())


def step_inputs(srcs, dsts, step_dev, step, flag_dev=None, flag=0):
    """ncn_step_inputs: copy each srcs[i] into dsts[i] (contiguous CUDA tensors of equal size), write
    `step` into the int64 device scalar step_dev and `flag` into the int32 flag_dev, in one launch."""
    n = len(srcs)
    VP = ctypes.c_void_p * max(n, 1)
    src = VP(*[s.data_ptr() for s in srcs])
    dst = VP(*[d.data_ptr() for d in dsts])
    nb = (ctypes.c_int64 * max(n, 1))(*[s.numel() * s.element_size() for s in srcs])
    return call("ncn_step_inputs", n, src, dst, nb, step_dev, int(step), flag_dev, int(flag))


def check_input(t, name):
    """The reference's CHECK_INPUT (models/csrc/include/utils.h:4-6)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def check_dtype(t, dtype, name):
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype} (got {t.dtype})")
