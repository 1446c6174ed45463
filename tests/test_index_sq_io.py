"""CPU: IndexScalarQuantizer's factory strings, refusals, IxSQ files and C names."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_index_sq")
FILES = ["sq8_l2_d40", "sq8_ip_d72", "sqfp16_l2_d24"]


@pytest.mark.parametrize("desc, cls, qtype, code_size, trained", [
    ("SQ8", "IndexScalarQuantizer", 0, 64, False),
    ("SQfp16", "IndexScalarQuantizer", 4, 128, True),
    ("SQ8,RFlat", "IndexRefineFlat", 0, 64, False),
    ("SQfp16,Refine(Flat)", "IndexRefineFlat", 4, 128, True),
])
def test_factory(amd, desc, cls, qtype, code_size, trained):
    idx = amd.index_factory(64, desc, amd.METRIC_INNER_PRODUCT)
    assert type(idx).__name__ == cls and idx.metric_type == amd.METRIC_INNER_PRODUCT
    sq = idx.base_index if cls == "IndexRefineFlat" else idx
    assert type(sq) is amd.IndexScalarQuantizer
    assert (sq.qtype, sq.code_size, sq.is_trained, sq.ntotal) == (qtype, code_size, trained, 0)
    assert sq.codes.shape == (0, code_size) and sq.sq_trained().size == 0


@pytest.mark.parametrize("desc, d, needle", [
    ("SQ4", 64, "QT_4bit"), ("SQ6", 64, "QT_6bit"), ("SQbf16", 64, "QT_bf16"),
    ("SQ8_direct", 64, r"QT_8bit_direct \("), ("SQ8_direct_signed", 64, "QT_8bit_direct_signed"),
    ("SQ8", 12, "d = 12"), ("SQfp16", 12, "d = 12"),
])
def test_refusals(amd, desc, d, needle):
    with pytest.raises(amd.FaissError, match=needle):
        amd.index_factory(d, desc)
    with pytest.raises(amd.FaissError, match=r"unsupported index_factory string LSH$"):
        amd.index_factory(d, "LSH")


def test_read_refuses_other_qtypes_and_dims(amd, tmp_path):
    blob = bytearray(open(os.path.join(GOLDEN, "sq8_l2_d40.faiss"), "rb").read())
    q4 = bytes(blob[:37]) + (1).to_bytes(4, "little") + bytes(blob[41:])  # sq.qtype
    (tmp_path / "q4.faiss").write_bytes(q4)
    with pytest.raises(amd.FaissError, match="QT_4bit"):
        amd.read_index(tmp_path / "q4.faiss")
    d12 = bytes(blob[:4]) + (12).to_bytes(4, "little") + bytes(blob[8:])  # the header's d
    (tmp_path / "d12.faiss").write_bytes(d12)
    with pytest.raises(amd.FaissError, match="d = 12"):
        amd.read_index(tmp_path / "d12.faiss")


@pytest.mark.parametrize("tag", FILES)
def test_ixsq_round_trip(amd, tmp_path, tag):
    src = os.path.join(GOLDEN, tag + ".faiss")
    idx = amd.read_index(src)
    assert type(idx) is amd.IndexScalarQuantizer and idx.ntotal == 300 and idx.is_trained
    assert idx.codes.shape == (300, idx.code_size)
    assert idx.sq_trained().size == (0 if "fp16" in tag else 2 * idx.d)
    for name, ix in (("read", idx), ("clone", amd.clone_index(idx))):
        assert type(ix) is amd.IndexScalarQuantizer
        amd.write_index(ix, tmp_path / name)
        assert (tmp_path / name).read_bytes() == open(src, "rb").read()


def test_train_and_add_give_the_reference_ranges_and_codes(amd):
    f = np.load(os.path.join(GOLDEN, "train_add.npz"))
    idx = amd.index_factory(f["x"].shape[1], "SQ8")
    idx.train(f["x"])
    idx.add(f["x"])
    assert idx.is_trained and idx.ntotal == len(f["x"])
    assert np.array_equal(idx.sq_trained().view(np.uint32), f["trained"].view(np.uint32))
    assert np.array_equal(idx.codes, f["codes"])


def test_range_search_throws_and_c_names(amd):
    idx = amd.read_index(os.path.join(GOLDEN, "sq8_l2_d40.faiss"))
    with pytest.raises(amd.FaissError, match="IndexScalarQuantizer: range search not implemented"):
        idx.range_search(np.zeros((1, 40), np.float32), 1.0)
    names = [s for s in amd.exported_symbols() if s.startswith("faiss_amd_IndexSQ_")]
    assert names == ["faiss_amd_IndexSQ_" + s for s in ("codes", "info", "set_content", "trained")]
    assert all(hasattr(amd.lib(), s) for s in names)
