"""The C ABI library: loads on CPU-only hosts and exports every symbol the headers of include/ declare
(no compute calls without a GPU); the ctypes binding and the package's constants are derived from
those headers through one registry (known answers, the parser's strictness, the loader's errors) and
`call` refuses a wrong argument before anything is launched."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest
import torch

from ncnerf_amd import _lib
from ncnerf_amd._lib import F32, F64, I32, I64, P, U32, U64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "ncnerf.h")
# each feature header's entry points, written out by hand (ncnerf.h: pinned at 80 below); the feature
# test files take their NAMES from here
NAMES = {
    "ncnerf_metrics.h": {"ncn_metrics_pointwise", "ncn_metrics_ssim", "ncn_metrics_angles", "ncn_select_median",
                         "ncn_metrics_finalise"},
    "ncnerf_geom.h": {"ncn_geom_loss_fwd", "ncn_geom_loss_bwd", "ncn_batch_labels_fw"},
    "ncnerf_mesh.h": {"ncn_mesh_points", "ncn_mesh_count", "ncn_mesh_scan", "ncn_mesh_emit_verts", "ncn_mesh_emit_faces"},
    "ncnerf_heads.h": {"ncn_head_packed_halves", "ncn_head_pack_weights", "ncn_head_fwd", "ncn_head_feat",
                       "ncn_head_bwd_blocks", "ncn_head_bwd", "ncn_head_reduce_wgrad", "ncn_composite_extra_fw",
                       "ncn_composite_extra_bw"},
    "ncnerf_sem.h": {"ncn_sem_confusion", "ncn_sem_finalise", "ncn_batch_semantics_fw"},
    "ncnerf_input_grad.h": {"ncn_field_bwd_mlp_rgb_din"},
}
STREAM_LAST = ("ncnerf_metrics.h", "ncnerf_geom.h", "ncnerf_mesh.h", "ncnerf_sem.h", "ncnerf_input_grad.h")


def declared_symbols(header="ncnerf.h"):
    return sorted(_lib.parse_header(open(os.path.join(INCLUDE, header)).read()))


def scanned_symbols(header="ncnerf.h"):
    """Independent of the parser: every `ncn_name(` of the header without comments and directives."""
    text = open(os.path.join(INCLUDE, header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)  # (#define NCN_FIELD_NW (... is no declaration)
    return sorted(set(m.group(1) for m in re.finditer(r"\b(ncn_\w+)\s*\(", text, flags=re.I)))


def altered_headers(tmp_path, header, text=None):
    """A copy of include/ in tmp_path with `header` replaced by `text` (None: left out): the directory."""
    for h in _lib.HEADERS:
        shutil.copy(os.path.join(INCLUDE, h), tmp_path)
    if text is None:
        os.remove(tmp_path / header)
    else:
        (tmp_path / header).write_text(text)
    return str(tmp_path)


def test_parser_and_scan_agree_on_the_symbols():
    syms = declared_symbols()
    assert syms == scanned_symbols()
    assert len(syms) == 80 == len(_lib.symbols("ncnerf.h"))
    assert {"ncn_morton3D", "ncn_morton3D_invert", "ncn_field_bwd_dE_floats"} <= set(syms)


# ---- the registry: one table from every header of HEADERS ----
def test_headers_are_the_files_of_include():
    assert set(_lib.HEADERS) == {f for f in os.listdir(INCLUDE) if f.endswith(".h")} and len(_lib.HEADERS) == 7
    assert _lib.HEADERS[0] == "ncnerf.h" and _lib.header_path("ncnerf.h") == HEADER and _lib.INCLUDE_DIR == INCLUDE


@pytest.mark.parametrize("header", _lib.HEADERS)
def test_each_header_parses_into_the_one_table(header):
    parsed = _lib.parse_header(open(os.path.join(INCLUDE, header)).read())
    assert sorted(parsed) == scanned_symbols(header) and set(parsed) == NAMES.get(header, set(parsed))
    assert _lib.symbols(header) == list(parsed)  # declaration order
    for name, decl in parsed.items():
        assert _lib.HEADER_OF[name] == header and _lib.ABI[name] == decl == _lib.declaration(name)
        assert len(_lib.SIGNATURES[name]) == len(decl[1])
    if header != "ncnerf.h":
        assert all(ret == "int" for ret, _ in parsed.values())
    if header in STREAM_LAST:
        assert all(params[-1] == ("ptr", 0, "stream") for _, params in parsed.values())


def test_symbols_is_the_concatenation_in_header_order():
    every = [name for header in _lib.HEADERS for name in _lib.symbols(header)]
    assert _lib.symbols() == every == list(_lib.ABI) == _lib.exported_symbols() == list(_lib.SIGNATURES)
    assert len(every) == len(set(every)) == 80 + sum(map(len, NAMES.values()))  # no name belongs to two headers
    assert _lib.load_headers() == (_lib.ABI, _lib.HEADER_OF, _lib.CONSTANTS, _lib.NON_LITERAL_DEFINES)
    with pytest.raises(KeyError):
        _lib.symbols("ncnerf_none.h")
    with pytest.raises(KeyError):
        _lib.declaration("ncn_none")


@pytest.mark.parametrize("header", _lib.HEADERS)
def test_clash_duplicate_and_missing_file(header, tmp_path):
    """load_headers on copies of the real headers with `header` altered: a name of another header in
    it is an NcnError naming both, a name twice in it parse_header's ValueError, and without the file
    the NcnError names its full path."""
    i = _lib.HEADERS.index(header)
    other = _lib.HEADERS[(i + 1) % len(_lib.HEADERS)]
    name, own = _lib.symbols(other)[0], _lib.symbols(header)[0]
    first, second = sorted((header, other), key=_lib.HEADERS.index)
    clash = altered_headers(tmp_path, header, f"int {own}(int a, void* stream);\nint {name}(void);\n")
    with pytest.raises(_lib.NcnError, match=re.escape(f"{name} is declared in include/{second} and in include/{first}")):
        _lib.load_headers(clash)
    twice = altered_headers(tmp_path, header, f"int {own}(int a, void* stream);\nint {own}(int b, void* stream);\n")
    with pytest.raises(ValueError, match=f"{own} is declared twice"):
        _lib.load_headers(twice)
    gone = altered_headers(tmp_path, header)
    with pytest.raises(_lib.NcnError, match=re.escape(os.path.join(gone, header)) + ".*derived from it"):
        _lib.load_headers(gone)
    with pytest.raises(_lib.NcnError, match=re.escape(os.path.join(gone, header))):
        _lib.read_header(header, gone)
    assert _lib.read_header(other, gone) == open(os.path.join(INCLUDE, other)).read()


# ---- the constants: every `#define NCN_<NAME> <literal>`, the values written out by hand ----
CONSTANTS = {
    "NCN_FIELD_PACKED_HALVES": 19456, "NCN_ENC_BYTES_PER_SAMPLE": 64, "NCN_PREC_F16": 0, "NCN_PREC_BF16": 1,
    "NCN_GEOM_DEPTH": 1, "NCN_GEOM_NORM_L1": 2, "NCN_GEOM_NORM_DOT": 4, "NCN_GEOM_REG": 8,
    "NCN_SEM_MAX_CLASSES": 64, "NCN_HEAD_MAX_OUT": 48, "NCN_HEAD_PACKED_HALVES": 16384, "NCN_EXTRA_MAX_CH": 51,
    "NCN_MESH_TILE_X": 32, "NCN_MESH_TILE_Y": 8, "NCN_MESH_TILE_Z": 8, "NCN_MESH_SCAN_ELEMS": 4096,
    "NCN_MESH_SCAN_SWEEP": 1024, "NCN_CORNER_REFERENCE": 0, "NCN_CORNER_GRID": 1, "NCN_IMAGE_F32": 0, "NCN_IMAGE_U8": 1,
    "NCN_AMP_INIT_SCALE": 65536.0, "NCN_TCNN_LOSS_SCALE": 128.0, "NCN_AMP_GROWTH_INTERVAL": 2000,
}
LEFT_OUT = {"NCN_FIELD_NW": "ncnerf.h", "NCN_HEAD_NW": "ncnerf_heads.h", "NCN_SSIM_TAPS": "ncnerf_metrics.h"}


def test_known_constants():
    assert _lib.CONSTANTS == CONSTANTS
    assert {k: type(v) for k, v in _lib.CONSTANTS.items()} == {k: type(v) for k, v in CONSTANTS.items()}
    assert set(_lib.NON_LITERAL_DEFINES) == set(LEFT_OUT) and len(_lib.NON_LITERAL_DEFINES) == 3
    assert all(_lib.HEADER_OF[k] == h for k, h in LEFT_OUT.items())
    assert _lib.HEADER_OF["NCN_GEOM_REG"] == "ncnerf_geom.h" and _lib.HEADER_OF["NCN_AMP_INIT_SCALE"] == "ncnerf.h"


def test_the_package_reads_its_constants_from_the_headers():
    from ncnerf_amd import data, losses, mesh, metrics, ngp_mt
    C = CONSTANTS
    assert ngp_mt.N_PACKED_HALVES == 19456 and ngp_mt.ENC_BYTES == 64 and ngp_mt.PRECISIONS == {"fp16": 0, "bf16": 1}
    assert ngp_mt.HEAD_MAX_OUT == 48 and ngp_mt.N_HEAD_PACKED_HALVES == 16384
    assert (losses.GEOM_DEPTH, losses.GEOM_NORM_L1, losses.GEOM_NORM_DOT, losses.GEOM_REG) == (1, 2, 4, 8)
    assert data.CORNER_MODES == {"reference": 0, "grid": 1} and data._IMAGE_DTYPES == {torch.float32: 0, torch.uint8: 1}
    assert metrics.MAX_SEM_CLASSES == 64 and _lib.AMP_INIT_SCALE == 65536.0 and type(_lib.AMP_INIT_SCALE) is float
    assert mesh.TILE == (32, 8, 8) and (mesh.SCAN_ELEMS, mesh.SCAN_SWEEP) == (4096, 1024)
    assert ngp_mt.N_W == 10240 and ngp_mt.head_nw(48) == 8192  # the two left-out formulas, restated in ngp_mt.py
    assert C["NCN_HEAD_MAX_OUT"] + 3 == C["NCN_EXTRA_MAX_CH"]


def test_parse_constants_takes_literals_only():
    values, left_out = _lib.parse_constants(
        "#ifndef NCNERF_X_H\n#define NCNERF_X_H\n/* #define NCN_GONE 1 */\n// #define NCN_GONE_TOO 2\n"
        "#define NCN_A 12 /* why */\n  #  define NCN_B -3\n#define NCN_C 1.5f\n#define NCN_D 2e3 // x\n#define NCN_E .25F\n"
        "#define NCN_F 0x10\n#define NCN_G (1 + 2)\n#define NCN_H(n) 4\n#define NCN_I { 1, 2 }\n#define NCN_J\n"
        "#define NCN_K 010\n#define NCN_L 7u\n#define OTHER 9\nint ncn_f(int NCN_M);\n#endif\n")
    assert values == {"NCN_A": 12, "NCN_B": -3, "NCN_C": 1.5, "NCN_D": 2000.0, "NCN_E": 0.25}
    assert [type(values[k]) for k in "NCN_A NCN_B NCN_C NCN_D NCN_E".split()] == [int, int, float, float, float]
    assert left_out == ["NCN_F", "NCN_G", "NCN_H", "NCN_I", "NCN_J", "NCN_K", "NCN_L"]
    with pytest.raises(ValueError, match="NCN_A is defined twice"):
        _lib.parse_constants("#define NCN_A 1\n#define NCN_A 1\n")


def test_a_constant_in_two_headers_is_an_error(tmp_path):
    clash = altered_headers(tmp_path, "ncnerf_sem.h", "#define NCN_SEM_MAX_CLASSES 64\n#define NCN_GEOM_REG 8\n")
    with pytest.raises(_lib.NcnError, match="NCN_GEOM_REG is declared in include/ncnerf_sem.h and in include/ncnerf_geom.h"):
        _lib.load_headers(clash)


def test_header_declares_the_hot_path():
    syms = declared_symbols()
    for s in ("ncn_ray_aabb_intersect", "ncn_march_train_walk", "ncn_march_train_scan", "ncn_march_train_pack",
              "ncn_composite_train_fw", "ncn_composite_train_bw", "ncn_field_fwd", "ncn_field_bwd", "ncn_field_sort_windows",
              "ncn_normals_fwd", "ncn_cluster_loss", "ncn_adam", "ncn_last_error"):
        assert s in syms


def test_library_exports_every_declared_symbol():
    """The raw library, every header's names; and lib() gives each its derived argtypes and restype."""
    L = ctypes.CDLL(_lib.LIB_PATH)
    declared = [s for header in _lib.HEADERS for s in declared_symbols(header)]
    missing = [s for s in declared if not hasattr(L, s)]
    assert not missing, missing
    assert len(declared) == 80 + sum(map(len, NAMES.values())) and set(declared) == set(_lib.exported_symbols())
    for name in declared:
        fn = getattr(_lib.lib(), name)
        assert list(fn.argtypes) == _lib.SIGNATURES[name] and fn.restype is _lib._RESTYPES[_lib.ABI[name][0]], name


def test_python_binding_covers_header():
    bound = set(_lib.exported_symbols())
    assert set(declared_symbols()) <= bound, set(declared_symbols()) - bound
    L = _lib.lib()
    assert L.ncn_version() >= 1
    assert L.ncn_last_error() is not None


def test_library_is_gfx950_code_object():
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in data


# ---- the derived binding: known answers, written out by hand ----
KNOWN = {
    # the list INTEGRATION.md §2 prints
    "ncn_composite_train_fw": [P, P, P, P, P, I64, I64, I32, F32, P, P, P, P, P, P],
    "ncn_batch_draw": [U64, P, I64, I32, I32, I32, I32, I64, I32, I32, P, P, P],
    "ncn_grid_packbits": [P, I64, F64, P, P, P, P],
    "ncn_adam_step_packed": [P, P, P, P, I64, I64, F32, F32, F32, F64, F64, F32, F32, F32, P, P, P, I32, P, P,
                             P, I64, P, I32, P],
    "ncn_kmeans_plan_fill": [I32, I32, U32, P],
    "ncn_step_inputs": [I32, P, P, P, P, I64, P, I32, P],
}
NON_INT = {"ncn_last_error": ctypes.c_char_p, "ncn_grid_work_bytes": I64, "ncn_march_train_fused_work_bytes": I64,
           "ncn_field_bwd_dE_floats": I64, "ncn_field_bwd_stash_floats": I64, "ncn_kmeans_plan_words": I64,
           "ncn_cluster_workspace_words": I64, "ncn_cluster_status_offset": I64, "ncn_adam_step_work_floats": I64}


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_argtypes(name):
    fn = getattr(_lib.lib(), name)
    assert _lib.SIGNATURES[name] == KNOWN[name]
    assert list(fn.argtypes) == KNOWN[name] and fn.restype is ctypes.c_int
    assert len(KNOWN["ncn_adam_step_packed"]) == 25 and KNOWN["ncn_adam_step_packed"].count(F64) == 2


def test_known_restypes():
    L = _lib.lib()
    got = {n: getattr(L, n).restype for n in _lib.exported_symbols() if getattr(L, n).restype is not ctypes.c_int}
    assert got == NON_INT


def test_parse_result_shape():
    abi = _lib.parse_header(open(HEADER).read())
    assert abi["ncn_morton3D"] == ("int", [("ptr", 4, "coords"), ("int64_t", 0, "n"), ("ptr", 4, "out"),
                                           ("ptr", 0, "stream")])
    assert abi["ncn_last_error"] == ("const char*", []) and abi["ncn_grid_work_bytes"] == ("int64_t", [])
    assert abi["ncn_step_inputs"][1][1:3] == [("ptr", 8, "src"), ("ptr", 8, "dst")]
    assert abi["ncn_field_fwd"][1][9] == ("ptr", 2, "weights_packed")


@pytest.mark.parametrize("header", [
    "int ncn_x(size_t n);",
    "int ncn_x(const float*);",
    "int ncn_x(int (*cb)(int));",
    "struct S ncn_x(int a);",
    "int ncn_x(int a)\nint ncn_y(int b);",
    "int ncn_x(int a)",
    "int ncn_x(inta);",
    "int ncn_x(float** a);",
    "unsigned ncn_x(int a);",
    "int ncn_x(int a); int ncn_x(int a);",
])
def test_parser_is_strict(header):
    with pytest.raises(ValueError, match="ncn_x"):
        _lib.parse_header(header)


def test_parser_accepts_the_grammar():
    abi = _lib.parse_header('/* c */\n#include <stdint.h>\nextern "C" {\nint64_t ncn_a(void);\n'
                            "const char* ncn_b(const void* const* p, double d /* why */, uint8_t *q); // x\n}\n")
    assert abi == {"ncn_a": ("int64_t", []),
                   "ncn_b": ("const char*", [("ptr", 8, "p"), ("double", 0, "d"), ("ptr", 1, "q")])}


# ---- marshalling: every refusal precedes the call, so none of this needs a GPU ----
@pytest.fixture
def streams(monkeypatch):
    """_lib.stream replaced by a counter: how often the current stream was fetched."""
    fetched = []

    def fake_stream():
        fetched.append(1)
        return P(0x5EED)
    monkeypatch.setattr(_lib, "stream", fake_stream)
    return fetched


def test_wrong_argument_count(streams):
    dev_like = P(16)
    for args in ((dev_like, 8), (dev_like, 8, dev_like, P(0), 1), ()):  # too few by two, too many, none
        with pytest.raises(TypeError, match=r"ncn_morton3D.*coords.*stream"):
            _lib.marshal("ncn_morton3D", args)
    with pytest.raises(TypeError, match="ncn_kmeans_plan_fill"):  # a host function has no stream to leave out
        _lib.marshal("ncn_kmeans_plan_fill", (1, 2, 3))
    assert not streams


def test_scalars(streams):
    buf = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(TypeError, match=r"ncn_kmeans_plan_fill: argument 0 \(n_tri\).*int.*float 3.0"):
        _lib.marshal("ncn_kmeans_plan_fill", (3.0, 2, 1234, buf))  # a float for an integer
    for tensor in (torch.tensor(3), torch.tensor([3]), torch.tensor(3.0)):  # a tensor for a scalar, int or float
        with pytest.raises(TypeError, match=r"argument 0 \(n_tri\)"):
            _lib.marshal("ncn_kmeans_plan_fill", (tensor, 2, 1234, buf))
        with pytest.raises(TypeError, match=r"ncn_packbits: argument 2 \(threshold\)"):
            _lib.marshal("ncn_packbits", (P(16), 8, tensor, P(16), P(0)))
    with pytest.raises(TypeError, match=r"argument 2 \(threshold\)"):
        _lib.marshal("ncn_packbits", (P(16), 8, "0.5", P(16), P(0)))
    out = _lib.marshal("ncn_packbits", (P(16), np.int64(8), 1, P(16), P(0)))  # index() and float() conversions
    assert type(out[1]) is int and out[1] == 8 and type(out[2]) is float and out[2] == 1.0
    assert _lib.marshal("ncn_kmeans_plan_fill", (True, 2, 1234, buf))[0] == 1
    assert not streams


def test_pointers(streams):
    i32, i64 = torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int64)
    # a host function takes CPU tensors of the pointee's width
    assert _lib.marshal("ncn_kmeans_plan_fill", (1, 2, 3, i32)) == (1, 2, 3, i32.data_ptr())
    with pytest.raises(TypeError, match=r"ncn_kmeans_plan_fill: argument 3 \(host_out\).*4-byte.*int64 cpu tensor"):
        _lib.marshal("ncn_kmeans_plan_fill", (1, 2, 3, i64))
    # a launching function takes CUDA tensors only, whichever pointer it is
    for args in ((i32, 8, P(16)), (P(16), 8, i32)):
        with pytest.raises(TypeError, match=r"ncn_morton3D: argument [02] \((coords|out)\).*CUDA.*cpu tensor"):
            _lib.marshal("ncn_morton3D", args)
    # the width is all that is checked: fp16 and bf16 both pass for uint16_t*, float32 for a uint32_t*
    # workspace, anything for void* (a host function of its own, so that CPU tensors are accepted)
    params = _lib.parse_header("int ncn_t(const uint16_t* h, uint32_t* w, const void* v, double* d);")["ncn_t"][1]
    fn, counts = _lib._marshaller("ncn_t", params)
    w, f64 = torch.zeros(2), torch.zeros(2, dtype=torch.float64)
    for h in (torch.zeros(2, dtype=torch.float16), torch.zeros(2, dtype=torch.bfloat16)):
        for v in (h, i32, f64, torch.zeros(2, dtype=torch.uint8)):
            assert fn(h, w, v, f64) == (h.data_ptr(), w.data_ptr(), v.data_ptr(), f64.data_ptr())
    assert counts == (4,)
    with pytest.raises(TypeError, match=r"argument 0 \(wire\).*2-byte"):
        _lib.marshal("ncn_grad_unpack_f16", (torch.zeros(2), 2, None, None))
    # a bare int and a numpy array are no pointers
    for bad in (i32.data_ptr(), np.zeros(8, np.int32), [1, 2], "x"):
        with pytest.raises(TypeError, match=r"argument 3 \(host_out\)"):
            _lib.marshal("ncn_kmeans_plan_fill", (1, 2, 3, bad))
    assert _lib.marshal("ncn_kmeans_plan_fill", (1, 2, 3, None))[3] is None  # NULL
    assert not streams


def test_ctypes_instances_pass_untouched(streams):
    arr = (ctypes.c_void_p * 2)()
    cap = ctypes.c_int(0)
    args = (I32(2), arr, ctypes.cast(arr, P), ctypes.byref(cap), P(None), I64(5), P(16), I32(1), P(0x77))
    out = _lib.marshal("ncn_step_inputs", args)
    assert len(out) == 9 and all(a is b for a, b in zip(out, args))
    args = (U64(1), P(None), I64(0), I32(1), I32(8), I32(8), I32(2), I64(4), I32(0), I32(0), P(16), P(16), P(0x77))
    assert all(a is b for a, b in zip(_lib.marshal("ncn_batch_draw", args), args))
    args = (P(16), I64(8), F64(0.5), P(16), P(16), P(16), P(0x77))
    assert all(a is b for a, b in zip(_lib.marshal("ncn_grid_packbits", args), args))
    assert _lib.marshal("ncn_packbits", (P(16), 8, F32(0.5), P(16), P(0)))[2].value == 0.5
    assert _lib.marshal("ncn_kmeans_plan_fill", (1, 2, U32(3), P(16)))[2].value == 3
    assert not streams  # full-length lists: used as given


def test_stream_appended_only_when_exactly_one_is_missing(streams):
    out = _lib.marshal("ncn_morton3D", (P(16), 8, P(32)))
    assert len(out) == 4 and out[3].value == 0x5EED and len(streams) == 1
    mine = P(0x77)
    assert _lib.marshal("ncn_morton3D", (P(16), 8, P(32), mine))[3] is mine and len(streams) == 1
    with pytest.raises(TypeError):
        _lib.marshal("ncn_morton3D", (P(16), 8.5, P(32)))  # refused before the stream is fetched
    assert len(streams) == 1


def test_a_refused_call_never_reaches_the_library(streams, monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was entered"))
    with pytest.raises(TypeError):
        _lib.call("ncn_morton3D", torch.zeros(8, 3, dtype=torch.int32), 8, torch.zeros(8, dtype=torch.int32))
    with pytest.raises(TypeError):
        _lib.call("ncn_kmeans_plan_fill", 1, 2, 3)
    assert not streams


def test_missing_header_names_the_path(tmp_path):
    with pytest.raises(_lib.NcnError, match=re.escape(str(tmp_path / "include" / "ncnerf.h"))):
        _lib.read_header("ncnerf.h", str(tmp_path / "include"))  # (no such directory)


@pytest.mark.gpu
def test_morton3D_through_call():
    """ncn_morton3D, 8 coordinates: the stream omitted == stream() passed; an int64 `coords` is a
    TypeError and launches nothing (the sentinel-filled output is untouched after a synchronise)."""
    dev = torch.device("cuda:0")
    coords = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [5, 9, 127], [127, 127, 127],
                           [64, 3, 77]], dtype=torch.int32, device=dev)
    a = torch.full((8,), -7, dtype=torch.int32, device=dev)
    b = torch.full((8,), -7, dtype=torch.int32, device=dev)
    _lib.call("ncn_morton3D", coords, 8, a)
    _lib.call("ncn_morton3D", coords, 8, b, _lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(a, b) and a[0] == 0 and a[4] == 7 and a[6] == 2 ** 21 - 1 and -7 not in a.tolist()
    out = torch.full((8,), -7, dtype=torch.int32, device=dev)
    with pytest.raises(TypeError, match=r"ncn_morton3D: argument 0 \(coords\)"):
        _lib.call("ncn_morton3D", coords.long(), 8, out)
    torch.cuda.synchronize()
    assert out.tolist() == [-7] * 8
