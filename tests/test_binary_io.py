"""Binary indexes without a GPU: the IBxF / IBwF file layout against files the
reference wrote (scripts/make_golden_binary.py), the factory strings, the named
refusals and the C header."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_binary")
INCLUDE = os.path.join(HERE, "..", "include")


@pytest.mark.parametrize("name,cls", [("flat", "IndexBinaryFlat"), ("ivf", "IndexBinaryIVF")])
def test_reference_files_round_trip(amd, tmp_path, name, cls):
    src = os.path.join(GOLDEN, name + ".faiss")
    idx = amd.read_index_binary(src)
    assert type(idx).__name__ == cls and idx.d == 16 and idx.ntotal == 300 and idx.is_trained
    if name == "ivf":
        assert idx.nlist == 8 and isinstance(idx.quantizer, amd.IndexBinaryFlat)
        assert idx.quantizer.ntotal == 8 and idx.use_heap
    amd.write_index_binary(idx, str(tmp_path / "out.faiss"))
    assert open(tmp_path / "out.faiss", "rb").read() == open(src, "rb").read()


def test_factory_strings(amd):
    flat = amd.index_binary_factory(64, "BFlat")
    assert isinstance(flat, amd.IndexBinaryFlat) and flat.d == 64 and flat.use_heap
    ivf = amd.index_binary_factory(64, "BIVF32")
    assert isinstance(ivf, amd.IndexBinaryIVF) and ivf.nlist == 32 and not ivf.is_trained
    assert ivf.nprobe == 1 and ivf.max_codes == 0 and ivf.use_heap
    assert isinstance(ivf.quantizer, amd.IndexBinaryFlat)
    with pytest.raises(amd.FaissError, match="unsupported"):
        amd.index_factory(64, "LSH")  # not routed through the float factory


@pytest.mark.parametrize("desc,word", [
    ("BIVF32_HNSW16", "IndexBinaryHNSW quantizer"), ("BHNSW16", "IndexBinaryHNSW"),
    ("BHash8", "IndexBinaryHash"), ("BHash4x8", "IndexBinaryHash"),
    ("BIVF32x", "did not generate"), ("Flat", "did not generate")])
def test_factory_refusals(amd, desc, word):
    with pytest.raises(amd.FaissError, match=word):
        amd.index_binary_factory(64, desc)
    with pytest.raises(amd.FaissError, match="multiple of 8"):
        amd.index_binary_factory(12, "BFlat")


@pytest.mark.parametrize("tag,kind", [(b"IBHf", "IndexBinaryHNSW"), (b"IBHh", "IndexBinaryHash"),
                                      (b"IBFf", "IndexBinaryFromFloat")])
def test_other_quantizers_refused_on_read(amd, tmp_path, tag, kind):
    b = open(os.path.join(GOLDEN, "ivf.faiss"), "rb").read()
    at = b.index(b"IBxF")  # the quantizer's record inside the IBwF file
    (tmp_path / "q.faiss").write_bytes(b[:at] + tag + b[at + 4:])
    with pytest.raises(amd.FaissError, match=kind):
        amd.read_index_binary(str(tmp_path / "q.faiss"))


def test_named_refusals(amd):
    xq = np.zeros((1, 2), np.uint8)
    flat = amd.read_index_binary(os.path.join(GOLDEN, "flat.faiss"))
    ivf = amd.read_index_binary(os.path.join(GOLDEN, "ivf.faiss"))
    with pytest.raises(amd.FaissError, match="search params not supported for this index"):
        flat.search(xq, 1, params=amd.SearchParametersIVF(nprobe=2))
    with pytest.raises(amd.FaissError, match="IndexBinaryFlat: range_search"):
        flat.range_search(xq, 3)
    with pytest.raises(amd.FaissError, match="IndexBinaryIVF: range_search"):
        ivf.range_search(xq, 3)
    with pytest.raises(amd.FaissError, match="IDSelector"):
        ivf.search(xq, 1, params=amd.SearchParametersIVF(nprobe=2, sel=amd.IDSelectorRange(0, 5)))
    with pytest.raises(amd.FaissError, match="store_pairs"):
        ivf.search_preassigned(xq, 1, np.zeros((1, 1), np.int64), store_pairs=True)
    with pytest.raises(amd.FaissError, match="merge_from"):
        ivf.merge_from(ivf)
    ivf.set_per_invlist_search(True)
    with pytest.raises(amd.FaissError, match="per_invlist_search"):
        ivf.search(xq, 1)
    with pytest.raises(amd.FaissError, match="65536"):
        amd.IndexBinaryFlat(65536 + 8)


def test_host_side_content(amd):
    ref = np.load(os.path.join(GOLDEN, "ref_binary.npz"))
    flat = amd.read_index_binary(os.path.join(GOLDEN, "flat.faiss"))
    assert np.array_equal(flat.reconstruct(7), ref["xb"][7])
    assert flat.remove_ids(amd.IDSelectorRange(0, 10)) == 10 and flat.ntotal == 290
    assert np.array_equal(flat.reconstruct(0), ref["xb"][10])
    ivf = amd.read_index_binary(os.path.join(GOLDEN, "ivf.faiss"))
    ivf.set_direct_map_type(2)  # Hashtable: the ids are not 0 .. ntotal - 1
    row = 5
    assert np.array_equal(ivf.reconstruct(int(ref["ids"][row])), ref["xb"][row])
    with pytest.raises(amd.FaissError):
        ivf.reconstruct(5)  # no such id
    ivf.reset()
    assert ivf.ntotal == 0


def test_c_header_compiles():
    for hdr in ("faiss_amd_c.h", os.path.join("faiss", "c_api", "IndexBinary_c.h")):
        subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", "-I", INCLUDE,
                        os.path.join(INCLUDE, hdr)], check=True)
