"""CPU: the public surface of the HNSW search parameters — the C++ struct
fields through the drop-in header <faiss/impl/HNSW.h>, the faiss_amd_* C
entry points, and the Python classes."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CXX_USER = r"""
#include <faiss/impl/HNSW.h>
#include <faiss/IndexHNSW.h>
#include <faiss/impl/IDSelector.h>
int main() {
    faiss::SearchParametersHNSW p;
    static_assert(sizeof(p.check_relative_distance) == sizeof(bool), "bool field");
    p.efSearch = 32;
    p.check_relative_distance = false;
    p.bounded_queue = false;
    faiss::IDSelectorRange r(0, 10);
    p.sel = &r;
    faiss::IndexHNSWFlat ix(16, 8);
    ix.hnsw.check_relative_distance = false;
    ix.hnsw.search_bounded_queue = false;
    // the reference's field order: efSearch, check_relative_distance, bounded_queue
    return (char*)&p.check_relative_distance < (char*)&p.bounded_queue &&
                           (char*)&p.efSearch < (char*)&p.check_relative_distance
                   ? 0
                   : 1;
}
"""

NEW_SYMBOLS = [
    "faiss_amd_SearchParametersHNSW_new",
    "faiss_amd_SearchParametersHNSW_free",
    "faiss_amd_SearchParametersIVF_set_quantizer_hnsw",
    "faiss_amd_SearchParametersIVF_set_quantizer_params",
    "faiss_amd_IndexHNSW_check_relative_distance",
    "faiss_amd_IndexHNSW_set_check_relative_distance",
    "faiss_amd_IndexHNSW_search_bounded_queue",
    "faiss_amd_IndexHNSW_set_search_bounded_queue",
    "faiss_amd_Index_search_device_with_params",
]


def test_reference_caller_sets_the_fields(tmp_path):
    src = tmp_path / "user.cpp"
    src.write_text(CXX_USER)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_new_symbols_exported_and_declared(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", amd.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    declared = set(amd.exported_symbols())
    for s in NEW_SYMBOLS:
        assert s in defined, s
        assert s in declared, s


def test_python_classes_round_trip(amd):
    p = amd.SearchParametersHNSW()
    assert (p.efSearch, p.check_relative_distance, p.bounded_queue, p.sel) == (16, True, True, None)
    sel = amd.IDSelectorRange(3, 9)
    p = amd.SearchParametersHNSW(efSearch=40, check_relative_distance=False, bounded_queue=False,
                                 sel=sel)
    assert (p.efSearch, p.check_relative_distance, p.bounded_queue) == (40, False, False)
    assert p.sel is sel and p.h
    ix = amd.IndexHNSWFlat(16, 8)
    assert ix.check_relative_distance is True and ix.search_bounded_queue is True
    ix.check_relative_distance = False
    assert ix.check_relative_distance is False and ix.search_bounded_queue is True
    ix.search_bounded_queue = False
    ix.check_relative_distance = True
    assert ix.check_relative_distance is True and ix.search_bounded_queue is False
    sp = amd.SearchParametersIVF(nprobe=4, quantizer_params=p)
    assert sp.quantizer_params is p
    assert amd.SearchParametersIVF(nprobe=4, quantizer_efSearch=32).quantizer_params is None
    with pytest.raises(ValueError):
        amd.SearchParametersIVF(nprobe=4, quantizer_efSearch=32, quantizer_params=p)


def test_c_params_object_new_and_free(amd):
    p = ctypes.c_void_p()
    assert amd.lib().faiss_amd_SearchParametersHNSW_new(ctypes.byref(p), 8, 0, 1, None) == 0
    assert p.value
    amd.lib().faiss_amd_SearchParametersHNSW_free(p)
