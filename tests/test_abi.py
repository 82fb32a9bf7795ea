"""CPU tier: the C-ABI library builds/loads, exports every symbol of include/avm.h, struct layouts
match the ctypes mirror, and the product refuses to run without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

from conftest import PKG, ROOT, mod


def test_library_exports_every_declared_symbol():
    lib_m = mod("lib")
    L = lib_m.lib()
    hdr = open(os.path.join(ROOT, "include", "avm.h")).read()
    declared = set(re.findall(r"\b(avm_[a-z_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(lib_m.EXPORTS), declared ^ set(lib_m.EXPORTS)
    for name in declared:
        assert hasattr(L, name), name


def test_prototype_table_matches_every_declaration_of_the_header(abi):
    """abi.PROTOTYPES against include/avm.h, function by function: the key, the argument count and the class of the return type."""
    from helpers import header_declarations

    decl = header_declarations()
    assert len(decl) == 51 and set(decl) <= set(abi.PROTOTYPES), set(decl) - set(abi.PROTOTYPES)
    for name, (ret, n_args) in decl.items():
        restype, argtypes = abi.PROTOTYPES[name]
        assert len(argtypes) == n_args, (name, len(argtypes), n_args)
        if ret in ("int", "int32_t"):
            assert restype is C.c_int, name                                  # (ctypes' default restype)
        elif ret == "void":
            assert restype is None, name
        elif ret == "const char *":
            assert restype is C.c_char_p, name
        else:
            assert ret.endswith("*") and restype is C.c_void_p, (name, ret)
    L = mod("lib").lib()
    for name in set(abi.PROTOTYPES) - set(decl):
        assert name.startswith("avm_debug_") and hasattr(L, name), name


def test_loaded_library_carries_the_tables_prototypes(abi):
    L = mod("lib").lib()
    for name, (restype, argtypes) in abi.PROTOTYPES.items():
        f = getattr(L, name)
        assert f.argtypes == argtypes and f.restype is restype, name


def _arrays_instances(buffers, synth):
    from helpers import blank_windows

    image = buffers.ImageArrays.from_maps([{3: (0.1, 0.2, 0.0, 0.0, 0.0, 0.0)}, {}], 4, with_td=True, prob=[{3: 0.5}, {}])
    msg = buffers.ReloMsgArrays.from_messages([None, None], 4)
    return [blank_windows(2), synth.make_windows(1, tracks="sparse", n_feat=8), image, buffers.SelectorState.alloc(2, 8), msg,
            buffers.ReloState.alloc(2, 4), buffers.PriorOutArrays.alloc(2), synth.make_fsel(1, horizon=2, n_cand=4, n_cloud=4, max_features=2),
            buffers.FselOutArrays.alloc(1, 2, want_min_gap=True), synth.make_align(1, 6)[0], buffers.AlignOutArrays.alloc(1, 6)]


def test_arrays_classes_describe_their_structs(abi):
    """Every *Arrays class with a STRUCT: F64 and I32 are the struct's pointer members, the dims of an instance its other members, and
    every array of an instance is a member (ImageArrays' `prob` apart: the array select_stream takes beside the struct)."""
    buffers, synth = mod("buffers"), mod("synth")
    classes = [c for c in vars(buffers).values() if isinstance(c, type) and issubclass(c, buffers._Arrays) and c.STRUCT is not None]
    assert len(classes) == 10
    instances = _arrays_instances(buffers, synth)
    assert {type(x) for x in instances} == set(classes)
    for cls in classes:
        pointers = {k for k, t in cls.STRUCT._fields_ if t in (abi.c_dp, abi.c_ip)}
        assert set(cls.F64) | set(cls.I32) == pointers and not set(cls.F64) & set(cls.I32), cls
        assert all(getattr(cls.STRUCT, k).size == C.sizeof(C.c_void_p) for k in pointers)
    for x in instances:
        fields = dict(type(x).STRUCT._fields_)
        assert all(k in fields and fields[k] not in (abi.c_dp, abi.c_ip) for k in x.dims), (type(x), x.dims)
        assert set(x.a) - {"prob"} <= set(type(x).F64) | set(type(x).I32), type(x)
        s = x.struct()
        assert all(getattr(s, k) == v for k, v in x.dims.items())
        assert all(bool(getattr(s, k)) == (x.a.get(k) is not None) for k in type(x).F64 + type(x).I32), type(x)   # absent / None: NULL


def test_horizon_in_takes_arrays_or_tensors_and_refuses_a_mix(abi):
    import numpy as np
    import torch

    P, rng = 3, np.random.default_rng(0)
    host = [rng.standard_normal((P, n)) for n in (3, 4, 3, 3, 3, 4, 3, 3)] + [np.arange(P), np.full(P, 0.05)]
    s = abi.horizon_in(5, *host)
    assert (s.mem, s.n_problems, s.horizon) == (abi.AVM_MEM_HOST, P, 5) and s._keep["nr_imu"].dtype == np.int32
    assert all(C.cast(getattr(s, k), C.c_void_p).value == v.ctypes.data for k, v in s._keep.items()) and len(s._keep) == 10
    tensors = [torch.from_numpy(a) for a in host]                            # (tensors in host memory: the pointers are what is checked)
    t = abi.horizon_in(5, *tensors)
    assert t.mem == abi.AVM_MEM_DEVICE and t._keep["nr_imu"].dtype == torch.int32 and t._keep["k_quat"].shape == (P, 4)
    assert all(C.cast(getattr(t, k), C.c_void_p).value == v.data_ptr() for k, v in t._keep.items())
    with pytest.raises(ValueError, match="mixed"):
        abi.horizon_in(5, *(tensors[:4] + host[4:]))


def test_struct_sizes_match_ctypes_mirror(abi):
    L = mod("lib").lib()
    out = (C.c_int * 8)()
    n = L.avm_debug_struct_sizes(out)
    assert n == 7
    exp = [abi.Options, abi.WindowBatch, abi.PriorOut, abi.SolveSummary, abi.FselBatch, abi.FselOut, abi.Config]
    assert [out[i] for i in range(7)] == [C.sizeof(t) for t in exp]
    import numpy as np

    assert abi.SUMMARY_DTYPE == np.dtype(abi.SolveSummary)
    assert abi.SUMMARY_DTYPE.itemsize == C.sizeof(abi.SolveSummary)
    assert [(k, abi.SUMMARY_DTYPE.fields[k][1]) for k in abi.SUMMARY_DTYPE.names] == [(k, getattr(abi.SolveSummary, k).offset) for k, _ in abi.SolveSummary._fields_]


def test_default_options_agree(abi, oracle):
    L = mod("lib").lib()
    a, b, c = abi.Options(), abi.Options(), abi.default_options()
    assert L.avm_default_options(C.byref(a)) == 0
    assert oracle.lib().avmo_default_options(C.byref(b)) == 0
    assert bytes(a) == bytes(b) == bytes(c)


def test_no_cpu_fallback_without_device():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib_m = mod("lib")
    with pytest.raises(lib_m.AvmError):
        lib_m.Context(0)


def test_product_package_never_touches_the_oracle():
    """No file of the shipped package may import, include, link or call anything under oracle/."""
    banned = re.compile(r"oracle_py|libavm_oracle|avmo_|#include\s+\"[^\"]*oracle|import\s+oracle|from\s+oracle")
    # the package, the public headers (C ABI + the C++ host side) and the measurement / profiling scripts
    for top in (os.path.join(ROOT, PKG), os.path.join(ROOT, "include"), os.path.join(ROOT, "scripts")):
        for dirpath, _, files in os.walk(top):
            for f in files:
                if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h", ".sh", "Makefile")):
                    txt = open(os.path.join(dirpath, f)).read()
                    assert not banned.search(txt), (dirpath, f, banned.search(txt).group(0))


def test_avm_create_refuses_a_caller_built_against_another_header(abi):
    """avm_config::abi_version: the structs carry no size fields, so a host compiled against an older avm.h - avm_fsel_out had three
    members before min_gap - is stopped at avm_create(), before any call reads its structs.  Checked first: no device needed."""
    import ctypes as C

    L = __import__("importlib").import_module("anticipated-vins-mono_amd.lib").lib()
    assert L.avm_abi_version() == abi.AVM_ABI_VERSION
    for stale in (0, abi.AVM_ABI_VERSION - 1, abi.AVM_ABI_VERSION + 1):
        cfg = abi.Config()
        cfg.abi_version = stale
        h = C.c_void_p()
        assert L.avm_create(C.byref(cfg), C.byref(h)) == abi.AVM_ERR_INVALID and not h.value
