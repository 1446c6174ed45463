"""METRIC_INNER_PRODUCT on IndexHNSWFlat, the parts that need no GPU.

tests/hnsw_ip_model.py (the Python restatement of HNSW::search over -<q, y>)
against every standalone case of the reference-run fixtures
(scripts/make_golden_hnsw_ip.py): D, I and the four HNSWStats deltas, bit for
bit.  The index files read and write back byte for byte, index_factory and
the constructor build an inner-product IndexHNSWFlat, and this library's host
add of a fixture's rows writes the reference's file byte for byte (levels,
offsets, neighbours, entry point: the graph built over -<q, y>).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hnsw_ip_model as im  # noqa: E402
from test_hnsw_params_model import member_of  # noqa: E402

FX = im.load_fixtures()


@pytest.fixture(scope="module")
def models(amd, orc):
    return {tag: im.Model(orc, orc.HNSWGraph.from_index(amd.read_index(fn)))
            for tag, fn in im.FILES.items()}


@pytest.mark.parametrize("tag", ["h16", "h8"])
def test_model_equals_reference(models, tag):
    m = models[tag]
    xq = FX[f"{tag}_xq"]
    js = im.jobs(FX, tag)
    assert len(js) == 50
    for name, k, how, ef, chk, bnd, sel, _ in js:
        assert how == "params"
        D, I, st = m.search(xq, k, ef, chk, bnd, member_of(sel, m.ntotal))
        im.assert_case(FX, f"{tag}_{name}", D, I, st)


def test_fixture_is_not_an_l2_search(amd, orc):
    """An L2 search of the same graph and rows gives other ids (what a kernel
    that ignored the metric would return)."""
    import hnsw_params_model as hm
    g = orc.HNSWGraph.from_index(amd.read_index(im.FILES["h16"]))
    _, I, _ = hm.Model(orc, g).search(FX["h16_xq"], 1, 200)
    assert (I[:, 0] != FX["h16_def_ef200_k1_I"][:, 0]).mean() >= 0.5


@pytest.mark.parametrize("fn", sorted({**im.FILES, **im.IVF_FILES}.values()))
def test_read_write_is_byte_identical(amd, tmp_path, fn):
    idx = amd.read_index(fn)
    assert idx.metric_type == amd.METRIC_INNER_PRODUCT
    q = getattr(idx, "quantizer", idx)
    assert type(q).__name__ == "IndexHNSWFlat" and q.metric_type == amd.METRIC_INNER_PRODUCT
    out = tmp_path / "o.faiss"
    amd.write_index(idx, out)
    assert out.read_bytes() == open(fn, "rb").read()


def test_constructor_and_factory_build_inner_product(amd):
    h = amd.IndexHNSWFlat(24, 16, amd.METRIC_INNER_PRODUCT)
    assert h.metric_type == amd.METRIC_INNER_PRODUCT and h.ntotal == 0
    f = amd.index_factory(24, "HNSW16,Flat", amd.METRIC_INNER_PRODUCT)
    assert type(f).__name__ == "IndexHNSWFlat" and f.metric_type == amd.METRIC_INNER_PRODUCT
    for desc in ("IVF64_HNSW8,Flat", "IVF64_HNSW8,PQ8", "IVF64_HNSW8,SQ8"):
        ivf = amd.index_factory(32, desc, amd.METRIC_INNER_PRODUCT)
        assert ivf.metric_type == amd.METRIC_INNER_PRODUCT
        assert ivf.quantizer.metric_type == amd.METRIC_INNER_PRODUCT


@pytest.mark.parametrize("tag,M", [("h16", 16), ("h8", 8)])
def test_host_add_writes_the_reference_file(amd, orc, tmp_path, tag, M):
    """The rows of the fixture, in one add as the reference added them, into
    an empty inner-product IndexHNSWFlat: the file is the reference's."""
    ref = amd.read_index(im.FILES[tag])
    xb = orc.idx_storage(ref)
    h = amd.IndexHNSWFlat(xb.shape[1], M, amd.METRIC_INNER_PRODUCT)
    h.add(xb)
    ep, ml, levels, offsets, neighbors, cum = h.graph()
    rep, rml, rlevels, roffsets, rneighbors, rcum = ref.graph()
    assert (ep, ml) == (rep, rml)
    np.testing.assert_array_equal(levels, rlevels)
    np.testing.assert_array_equal(offsets, roffsets)
    np.testing.assert_array_equal(neighbors, rneighbors)
    out = tmp_path / "o.faiss"
    amd.write_index(h, out)
    assert out.read_bytes() == open(im.FILES[tag], "rb").read()
