"""IndexPQ without a GPU: factory strings, the refused widths and search types,
and the IxPq file layout against a file the reference wrote
(scripts/make_golden_index_pq.py)."""
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_index_pq")


@pytest.mark.parametrize("desc,cls,M,nbits,code_size", [
    ("PQ8", "IndexPQ", 8, 8, 8), ("PQ16x6", "IndexPQ", 16, 6, 12), ("PQ5x5", "IndexPQ", 5, 5, 4),
    ("PQ8,RFlat", "IndexRefineFlat", 8, 8, 8), ("PQ8x4,Refine(Flat)", "IndexRefineFlat", 8, 4, 4),
    ("OPQ8,PQ8", "IndexPreTransform", 8, 8, 8),
])
def test_factory_strings(amd, desc, cls, M, nbits, code_size):
    idx = amd.index_factory(80, desc)
    assert type(idx).__name__ == cls and idx.d == 80 and not idx.is_trained
    pq = {"IndexPQ": lambda: idx, "IndexRefineFlat": lambda: idx.base_index,
          "IndexPreTransform": lambda: idx.index}[cls]()
    assert isinstance(pq, amd.IndexPQ) and pq.ntotal == 0
    assert pq.pq_info() == dict(M=M, nbits=nbits, code_size=code_size, search_type=amd.ST_PQ)


@pytest.mark.parametrize("desc,word", [("PQ8x3", "nbits = 3"), ("PQ8x9", "nbits = 9"),
                                       ("PQ8x8z", "unsupported PQ spec"), ("PQ7", "multiple")])
def test_factory_refusals(amd, desc, word):
    with pytest.raises(amd.FaissError, match=word):
        amd.index_factory(40, desc)


@pytest.mark.parametrize("st,name", [(1, "ST_HE"), (2, "ST_generalized_HE"), (3, "ST_SDC"),
                                     (4, "ST_polysemous"), (5, "ST_polysemous_generalize")])
def test_other_search_types_refused_by_name(amd, st, name):
    import numpy as np
    idx = amd.read_index(os.path.join(GOLDEN, "pq5x5_l2.faiss"))
    xq = np.zeros((1, idx.d), np.float32)
    with pytest.raises(amd.FaissError, match=name + " is not supported"):
        idx.search(xq, 1, params=amd.SearchParametersPQ(search_type=st))
    idx.search_type = st
    with pytest.raises(amd.FaissError, match=name + " is not supported"):
        idx.search(xq, 1)
    with pytest.raises(amd.FaissError, match="range search not implemented"):
        idx.range_search(xq, 1.0)


@pytest.mark.parametrize("tag,metric", [("pq8x8_l2", 1), ("pq12x6_ip", 0), ("pq5x5_l2", 1)])
def test_ixpq_bytes(amd, tmp_path, tag, metric):
    src = os.path.join(GOLDEN, tag + ".faiss")
    idx = amd.read_index(src)
    assert isinstance(idx, amd.IndexPQ) and idx.is_trained and idx.metric_type == metric
    assert idx.codes.shape == (idx.ntotal, idx.code_size) and idx.ntotal == 300
    blob = open(src, "rb").read()
    for ix in (idx, amd.clone_index(idx)):
        amd.write_index(ix, str(tmp_path / "out.faiss"))
        assert open(tmp_path / "out.faiss", "rb").read() == blob
    # the two old tags stored METRIC_INNER_PRODUCT while searching L2; IxPQ
    # ends after the codes
    old = os.path.join(GOLDEN, "pq12x6_ip.faiss")
    for old_tag, cut in ((b"IxPo", 0), (b"IxPQ", 9)):
        b = open(old, "rb").read()
        (tmp_path / "old.faiss").write_bytes(old_tag + b[4:len(b) - cut])
        assert amd.read_index(str(tmp_path / "old.faiss")).metric_type == amd.METRIC_L2
