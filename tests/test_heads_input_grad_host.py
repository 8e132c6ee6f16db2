"""Host side of the input gradients with a head: the seventh ABI header (include/ncnerf_input_grad.h,
one entry point, ncn_field_bwd_mlp_rgb_din), its binding, the library's export of it, and the refusals
that precede the library.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from ncnerf_amd import _lib
from test_abi import altered_headers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "ncnerf_input_grad.h"
NAME = "ncn_field_bwd_mlp_rgb_din"
P, I64, I32 = _lib.P, _lib.I64, _lib.I32


def test_header_declares_the_entry_point_in_the_grammar():
    """(what every header shares, its names among it, is in test_abi.py)"""
    assert _lib.header_path(HEADER) == os.path.join(ROOT, "include", HEADER)
    seventh = _lib.parse_header(_lib.read_header(HEADER))
    assert set(seventh) == {NAME} and _lib.symbols(HEADER) == [NAME]
    ret, params = seventh[NAME]
    assert ret == "int" and params[-1] == ("ptr", 0, "stream")
    assert [p[2] for p in params] == ["xyzs", "dirs", "n", "n_dev", "order", "weights_packed", "precision", "enc_cache",
                                      "dL_drgbs", "loss_scale", "n_blocks", "slab", "dE_ws", "level_max", "dh_stash",
                                      "w_master", "dL_ddirs", "stream"]
    assert params[1] == ("ptr", 4, "dirs") and params[5] == ("ptr", 2, "weights_packed") and params[16] == ("ptr", 4, "dL_ddirs")
    assert _lib.SIGNATURES[NAME] == [P, P, I64, P, P, P, I32, P, P, P, I32, P, P, P, P, P, P, P]
    assert _lib.declaration(NAME) == seventh[NAME]
    # the arguments are part 1's of ncn_field_bwd_mlp_part (without the sigma terms and `part`), then
    # ncn_field_bwd_mlp_din's two last
    part = [p for p in _lib.declaration("ncn_field_bwd_mlp_part")[1] if p[2] not in ("dL_dsigmas", "dL_dsigmas2", "part")]
    din = _lib.declaration("ncn_field_bwd_mlp_din")[1]
    assert params == part[:-1] + din[-3:-1] + [part[-1]]


def test_library_exports_the_entry_point():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, NAME)
    fn = getattr(_lib.lib(), NAME)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.SIGNATURES[NAME]


def test_name_clash_and_missing_header(tmp_path):
    clash = altered_headers(tmp_path, HEADER, "int ncn_field_bwd_mlp_din(const float* xyzs, void* stream);\n")
    with pytest.raises(_lib.NcnError, match="ncn_field_bwd_mlp_din is declared in include/ncnerf_input_grad.h and in "
                                            "include/ncnerf.h"):
        _lib.load_headers(clash)
    gone = altered_headers(tmp_path, HEADER)
    with pytest.raises(_lib.NcnError, match=re.escape(os.path.join(gone, HEADER)) + ".*direction gradient"):
        _lib.load_headers(gone)


def _args(**over):
    d = _lib.P(16)
    a = dict(xyzs=d, dirs=d, n=16, n_dev=None, order=None, weights_packed=d, precision=0, enc_cache=d, dL_drgbs=d,
             loss_scale=None, n_blocks=0, slab=d, dE_ws=d, level_max=d, dh_stash=d, w_master=d, dL_ddirs=d)
    a.update(over)
    return tuple(a.values())


def test_refusals_precede_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "stream", lambda: _lib.P(0x5EED))
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was entered"))
    host_f32, host_f16 = torch.zeros(48), torch.zeros(48, dtype=torch.float16)
    with pytest.raises(TypeError, match=rf"{NAME}: argument 1 \(dirs\).*CUDA.*cpu tensor"):  # a host tensor
        _lib.call(NAME, *_args(dirs=host_f32))
    with pytest.raises(TypeError, match=rf"{NAME}: argument 16 \(dL_ddirs\).*4-byte"):  # a wrong width
        _lib.call(NAME, *_args(dL_ddirs=host_f16))
    with pytest.raises(TypeError, match=rf"{NAME}: argument 5 \(weights_packed\).*2-byte"):
        _lib.call(NAME, *_args(weights_packed=host_f32))
    with pytest.raises(TypeError, match=rf"{NAME}: argument 10 \(n_blocks\)"):
        _lib.call(NAME, *_args(n_blocks=1.0))
    with pytest.raises(TypeError, match=rf"{NAME}: takes 17 or 18 arguments, got 16"):
        _lib.call(NAME, *_args()[:-1])
    # what passes: NULLs and raw pointers, the current stream appended last
    out = _lib.marshal(NAME, _args())
    assert len(out) == 18 and out[3] is None and out[-1].value == 0x5EED
