"""IndexPreTransform without a GPU: factory prefixes, the limits' messages,
file round trips (IxPT and the VectorTransform records) and the C API's
IndexIVF accessors seen through the wrapper."""
import os
import struct

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_pretransform")


@pytest.mark.parametrize("desc,chain,sub", [
    ("OPQ8,IVF16,PQ8", [("OPQMatrix", 40, 40)], ("IndexIVFPQ", 40)),
    ("OPQ8_32,IVF16,PQ8", [("OPQMatrix", 40, 32)], ("IndexIVFPQ", 32)),
    ("PCA24,IVF16,Flat", [("PCAMatrix", 40, 24)], ("IndexIVFFlat", 24)),
    ("PCAR24,Flat", [("PCAMatrix", 40, 24)], ("IndexFlat", 24)),
    ("PCAW24,IVF16,SQ8", [("PCAMatrix", 40, 24)], ("IndexIVFScalarQuantizer", 24)),
    ("PCAWR16,HNSW8", [("PCAMatrix", 40, 16)], ("IndexHNSWFlat", 16)),
    ("RR36,IVF16,Flat", [("RandomRotationMatrix", 40, 36)], ("IndexIVFFlat", 36)),
    ("PCA32,OPQ8_24,IVF16,PQ8,RFlat", [("PCAMatrix", 40, 32), ("OPQMatrix", 32, 24)],
     ("IndexRefineFlat", 24)),
])
def test_factory_prefixes(amd, desc, chain, sub):
    idx = amd.index_factory(40, desc)
    assert isinstance(idx, amd.IndexPreTransform) and idx.d == 40 and idx.own_fields
    assert [(t.type_name, t.d_in, t.d_out) for t in idx.chain] == chain
    assert (type(idx.index).__name__, idx.index.d) == sub
    assert not idx.is_trained and not any(t.is_trained for t in idx.chain)


@pytest.mark.parametrize("desc,kind", [("OPQ8,IVF16,PQ8", "OPQMatrix"),
                                       ("PCA24,IVF16,Flat", "PCAMatrix"),
                                       ("RR24,Flat", "RandomRotationMatrix")])
def test_training_is_not_served(amd, desc, kind):
    idx = amd.index_factory(40, desc)
    with pytest.raises(amd.FaissError, match=f"training {kind} is not served; read a trained "
                                             "transform or set A"):
        idx.train(np.zeros((100, 40), np.float32))


def user_filled(amd):
    rng = np.random.default_rng(3)
    lt = amd.LinearTransform(A=rng.standard_normal((32, 40)).astype(np.float32),
                             b=rng.standard_normal(32).astype(np.float32))
    base = amd.index_factory(32, "IVF16,PQ8")
    return amd.IndexPreTransform(lt, base), lt, base


def test_write_read_round_trip(amd, tmp_path):
    idx, lt, _ = user_filled(amd)
    f1, f2 = str(tmp_path / "a.faiss"), str(tmp_path / "b.faiss")
    amd.write_index(idx, f1)
    back = amd.read_index(f1)
    amd.write_index(back, f2)
    raw = open(f1, "rb").read()
    assert raw[:4] == b"IxPT" and raw == open(f2, "rb").read()
    t, = back.chain
    assert (t.type_name, t.d_in, t.d_out, t.is_trained, t.have_bias) == \
        ("LinearTransform", 40, 32, True, True)
    assert np.array_equal(t.A, lt.A) and np.array_equal(t.b, lt.b) and not t.is_orthonormal
    assert isinstance(back.index, amd.IndexIVFPQ) and back.own_fields


def test_other_transform_kinds_are_rejected_by_name(amd, tmp_path):
    raw = bytearray(open(_written(amd, tmp_path), "rb").read())
    at = raw.index(b"LTra")
    for tag, kind in ((b"Viqt", "ITQTransform"), (b"Viqm", "ITQMatrix"),
                      (b"VNrm", "NormalizationTransform")):
        raw[at:at + 4] = tag
        path = tmp_path / "other.faiss"
        path.write_bytes(raw)
        with pytest.raises(amd.FaissError, match=kind):
            amd.read_index(str(path))


def _written(amd, tmp_path):
    path = str(tmp_path / "w.faiss")
    amd.write_index(user_filled(amd)[0], path)
    return path


def test_ivf_accessors_see_through_the_wrapper(amd):
    idx, _, base = user_filled(amd)
    L = amd.lib()
    assert L.faiss_IndexIVF_nlist(idx.h) == 16
    L.faiss_IndexIVF_set_nprobe(idx.h, 5)
    assert base.nprobe == 5 and L.faiss_IndexIVF_nprobe(idx.h) == 5
    amd.ParameterSpace().set_index_parameter(idx, "nprobe", 7)
    assert base.nprobe == 7
    assert L.faiss_IndexIVF_quantizer(idx.h) == L.faiss_IndexIVF_quantizer(base.h)
    flat = amd.IndexPreTransform(amd.LinearTransform(A=np.eye(8, dtype=np.float32)),
                                 amd.IndexFlatL2(8))
    with pytest.raises(amd.FaissError, match="not an IndexIVF"):
        amd.ParameterSpace().set_index_parameter(flat, "nprobe", 3)


def test_reference_files_round_trip(amd, tmp_path):
    for tag in ("opq8_32_ivf16_pq8", "pca24_ivf16_flat"):
        src = os.path.join(GOLDEN, tag + ".faiss")
        idx = amd.read_index(src)
        out = str(tmp_path / (tag + ".faiss"))
        amd.write_index(idx, out)
        assert open(src, "rb").read() == open(out, "rb").read(), tag
        assert isinstance(idx, amd.IndexPreTransform) and idx.is_trained and idx.d == 40
