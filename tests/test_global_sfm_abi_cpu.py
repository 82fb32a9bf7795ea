"""CPU tier: the second public header include/avm_init.h (the initialisation phase) against the Python mirror - its one declaration, the
layout of its two structs, the exported symbol - and include/avm.h untouched beside it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT, mod

INIT_H = os.path.join(ROOT, "include", "avm_init.h")


def _code():
    code = re.sub(r"/\*.*?\*/", "", open(INIT_H).read(), flags=re.S)
    return re.sub(r"^\s*#.*$", "", code, flags=re.M)


def test_header_declares_exactly_the_entry_point():
    abi, lib_m = mod("abi"), mod("lib")
    decl = re.findall(r"\b(avm_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", _code())
    assert [d[0] for d in decl] == ["avm_global_sfm_batch"] == list(abi.PROTOTYPES_INIT) == lib_m.EXPORTS_INIT
    n_args = len([x for x in decl[0][1].split(",") if x.strip()])
    restype, argtypes = abi.PROTOTYPES_INIT["avm_global_sfm_batch"]
    assert len(argtypes) == n_args == 6 and restype is C.c_int
    assert not set(abi.PROTOTYPES_INIT) & set(abi.PROTOTYPES)


def test_avm_h_keeps_its_version_and_does_not_declare_it():
    hdr = open(os.path.join(ROOT, "include", "avm.h")).read()
    assert "#define AVM_ABI_VERSION 6" in hdr and "avm_global_sfm_batch" not in hdr and "avm_sfm_batch" not in hdr
    assert mod("abi").AVM_ABI_VERSION == 6
    assert '#include "avm.h"' in open(INIT_H).read()


def test_library_exports_the_symbol_with_the_table_s_prototype():
    abi = mod("abi")
    L = mod("lib").lib()
    f = L.avm_global_sfm_batch
    assert f.restype is C.c_int and list(f.argtypes) == abi.PROTOTYPES_INIT["avm_global_sfm_batch"][1]


def test_struct_layouts_match_the_ctypes_mirrors(tmp_path):
    """sizeof / offsetof of avm_sfm_batch and avm_sfm_out from a compiled probe (C, the header as a C compiler sees it)"""
    abi = mod("abi")
    pairs = [("avm_sfm_batch", abi.SfmBatch), ("avm_sfm_out", abi.SfmOut)]
    lines = []
    for cname, S in pairs:
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        lines += ['printf("%%zu\\n", offsetof(%s, %s));' % (cname, f) for f, _ in S._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "avm_init.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for _, S in pairs:
        want += [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]
    assert got == want
    # the member names, in order, are the header's
    for cname, S in pairs:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), _code(), flags=re.S).group(1)
        names = re.findall(r"[\*\s,]([A-Za-z_]\w*)\s*(?=[,;])", body)
        assert names == [f for f, _ in S._fields_], (cname, names)


def test_arrays_hand_over_their_own_pointers():
    ib, synth, buffers = mod("init_buffers"), mod("synth"), mod("buffers")
    sf = synth.make_sfm(2, [(0, 11, 12)])[0]
    assert not hasattr(buffers.SfmArrays, "STRUCT") or buffers.SfmArrays.STRUCT is None  # the container of buffers.py stays as it was
    x = ib.SfmBatchArrays.of(sf)
    s = x.struct()
    assert (s.n_windows, s.max_frames, s.max_pts, s.ba_max_num_iterations, s.ba_max_solver_time_s) == (
        2, sf.dims["max_frames"], sf.dims["max_pts"], 50, 0.0)
    assert sorted(type(x).F64 + type(x).I32) == sorted(sf.a)
    for k, v in sf.a.items():
        assert x.a[k] is v and C.cast(getattr(s, k), C.c_void_p).value == v.ctypes.data, k
    o = ib.SfmOutArrays.alloc(2, 16, 40, want_chain=False)
    so = o.struct()
    assert o.n_windows == 2 and not so.pnp_q and not so.pnp_t
    for k, v in o.a.items():
        assert C.cast(getattr(so, k), C.c_void_p).value == v.ctypes.data, k
    assert o.a["frame_R"].shape == (2, 16, 9) and o.a["point"].shape == (2, 40, 3) and o.a["point_state"].dtype == np.int32
    assert set(ib.SfmOutArrays.alloc(1, 11, 4).a) == {f for f, _ in mod("abi").SfmOut._fields_}
