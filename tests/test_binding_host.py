"""
The Python binding against include/cip.h, without a GPU: every prototype of
the header against `_lib.PROTOTYPES` parameter by parameter, the four struct
mirrors field by field, and the call helpers of `_call` (NULL rule, dtype
codes, tensor checks, the invert flag word) on CPU tensors.
"""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from ska_sdp_cip_amd import _call, _lib, gridder

HEADER = Path(__file__).resolve().parents[1] / "include" / "cip.h"
MIRRORS = {"cip_gridder_params": _lib.GridderParams, "cip_clean_result": _lib.CleanResult,
           "cip_weight_grid": _lib.WeightGrid, "cip_weight_info": _lib.WeightInfo}
SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "double": ctypes.c_double}


@pytest.fixture(scope="module")
def header():
    text = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _prototypes(header):
    """name -> (return type, [parameter declarations]) of every cip_* function."""
    out = {}
    for ret, name, params in re.findall(r"\b(int|const\s+char\s*\*)\s*(cip_\w+)\s*\(([^)]*)\)\s*;", header):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = ("int" if ret == "int" else "str", [] if params == ["void"] else params)
    return out


def _matches(decl, argtype):
    """A C parameter declaration against the ctypes type the table gives it."""
    if "*" in decl:
        base = decl.replace("const", " ").split("*")[0].strip()
        if base in MIRRORS:
            return argtype is ctypes.POINTER(MIRRORS[base])
        return argtype is ctypes.c_void_p or issubclass(argtype, ctypes._Pointer)  # pylint: disable=protected-access
    base = decl.replace("const", " ").split()[0]
    return argtype is SCALARS[base]


def test_every_prototype_matches_the_table(header):
    protos = _prototypes(header)
    assert len(protos) == 41
    assert tuple(protos) == _lib.EXPORTED_SYMBOLS == tuple(_lib.PROTOTYPES)  # the header's names, in its order
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is (ctypes.c_int if ret == "int" else ctypes.c_char_p), name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (decl, argtype) in enumerate(zip(params, argtypes)):
            assert _matches(decl, argtype), (name, k, decl, argtype)


def test_lib_applies_the_table_to_every_symbol():
    so = _lib.lib()
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        fn = getattr(so, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert so.cip_release_workspace.argtypes == []  # parameterless symbols are declared too


def test_struct_mirrors_match_the_header(header):
    structs = dict(re.findall(r"typedef\s+struct\s+(cip_\w+)\s*\{(.*?)\}\s*\1\s*;", header, flags=re.S))
    assert set(structs) == set(MIRRORS)
    for name, body in structs.items():
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            ctype, names = decl.split(" ", 1)
            fields += [(n.strip(), SCALARS[ctype]) for n in names.split(",")]
        assert fields == list(MIRRORS[name]._fields_), name  # pylint: disable=protected-access


def test_ptr_is_null_for_none_and_empty():
    assert _call.ptr(None) is None
    assert _call.ptr(torch.empty(0)) is None
    assert _call.ptr(torch.zeros(4)[2:2]) is None  # an empty view of live storage
    t = torch.zeros(3)
    assert _call.ptr(t) == t.data_ptr() != 0


def test_vis_and_wgt_args():
    assert _call.vis_arg(None) == (None, _lib.CIP_C64)
    assert _call.wgt_arg(None) == (None, _lib.CIP_NONE)
    for dtype, code in ((torch.complex64, _lib.CIP_C64), (torch.complex128, _lib.CIP_C128)):
        t = torch.zeros(2, dtype=dtype)
        assert _call.vis_arg(t) == (t.data_ptr(), code)
        assert _call.vis_arg(t[:0]) == (None, code)
    for dtype, code in ((torch.float32, _lib.CIP_F32), (torch.float64, _lib.CIP_F64)):
        t = torch.zeros(2, dtype=dtype)
        assert _call.wgt_arg(t) == (t.data_ptr(), code)
    with pytest.raises(ValueError, match="vis dtype must be complex64/complex128, got torch.float32"):
        _call.vis_arg(torch.zeros(2))
    with pytest.raises(ValueError, match="wgt dtype must be float32/float64, got torch.int32"):
        _call.wgt_arg(torch.zeros(2, dtype=torch.int32))


def test_dtype_codes_equal_the_header(header):
    defines = dict(re.findall(r"#define\s+(CIP_\w+)\s+\(?(-?\d+)\)?", header))
    for name in ("CIP_NONE", "CIP_C64", "CIP_C128", "CIP_F32", "CIP_F64"):
        assert getattr(_lib, name) == int(defines[name]), name


def test_check_tensor_refuses_cpu_and_strided_tensors():
    with pytest.raises(ValueError, match="contiguous device tensors"):
        _call.check_tensor(torch.zeros(4), torch.device("cuda", 0), "x")
    strided = torch.zeros((4, 4)).t()
    assert not strided.is_contiguous()
    with pytest.raises(ValueError, match="contiguous device tensors"):
        _call.check_tensor(strided, strided.device, "x")
    with pytest.raises(ValueError):
        _call.check_array(torch.zeros(4), (torch.float64,), (4,), torch.device("cpu"), "x")  # dtype
    with pytest.raises(ValueError):
        _call.check_rows(torch.zeros((5, 3), dtype=torch.float64), torch.zeros(2, dtype=torch.float64), "x")  # CPU


def test_invert_flag_word_of_each_keyword(header):
    defines = dict(re.findall(r"#define\s+(CIP_\w+)\s+\(?(-?\d+)\)?", header))
    off = dict(do_wstacking=False, single_precision_accumulation=False, psf=False, normalise=False, synchronize=True,
               resident_inputs=False, reuse_plan=False)
    assert gridder._invert_flags(**off) == 0  # pylint: disable=protected-access
    for keyword, define in (("do_wstacking", "CIP_WSTACKING"), ("single_precision_accumulation", "CIP_ACC_SINGLE"),
                            ("psf", "CIP_PSF"), ("normalise", "CIP_NORMALISE"), ("synchronize", "CIP_ASYNC"),
                            ("resident_inputs", "CIP_PIPELINE"), ("reuse_plan", "CIP_REUSE_PLAN")):
        word = gridder._invert_flags(**{**off, keyword: not off[keyword]})  # pylint: disable=protected-access
        assert word == int(defines[define]), keyword
