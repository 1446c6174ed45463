"""IndexIVFScalarQuantizer on the host side: the reference's IwSq files
(tests/golden/ref_sq, written by the reference's write_index through
scripts/make_golden_sq.py) read, describe themselves and write back byte for
byte; index_factory builds the class; everything outside QT_8bit / QT_fp16 with
d % 8 == 0 is rejected with the qtype / d in the message.  No GPU needed."""
import os
import struct

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "ref_sq")
TAGS = ["sq8_l2_d64", "sq8_l2_d72", "sqfp16_l2_d64", "sq8_ip_d64", "sq8_hnsw_d64"]
QT_8bit, QT_4bit, QT_fp16 = 0, 1, 4


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "ref_sq.npz"))


def path(tag):
    return os.path.join(GOLD, tag + ".faiss")


@pytest.mark.parametrize("tag", TAGS)
def test_read_describe(amd, fx, tag):
    d, nlist, nb, _, ml2, code_size = (int(v) for v in fx[f"{tag}_meta"][:6])
    idx = amd.read_index(path(tag))
    assert type(idx) is amd.IndexIVFScalarQuantizer
    assert (idx.d, idx.nlist, idx.ntotal, idx.code_size) == (d, nlist, nb, code_size)
    assert idx.metric_type == (amd.METRIC_L2 if ml2 else amd.METRIC_INNER_PRODUCT)
    assert idx.is_trained and idx.by_residual
    fp16 = tag.startswith("sqfp16")
    assert idx.qtype == (QT_fp16 if fp16 else QT_8bit)
    tr = idx.sq_trained()
    assert tr.dtype == np.float32 and tr.size == (0 if fp16 else 2 * d)
    if not fp16:
        assert (tr[d:] >= 0).all()  # vdiff = vmax - vmin
    sizes = [idx.get_list_size(l) for l in range(nlist)]
    assert sum(sizes) == nb and max(sizes) > 64  # lists cross the 64-row tile
    ids = np.concatenate([idx.list_ids(l) for l in range(nlist)])
    assert np.array_equal(np.sort(ids), np.arange(nb, dtype=np.int64) * 3 + 7)
    assert idx.list_codes(0).shape == (sizes[0], code_size)
    q = idx.quantizer
    assert type(q) is (amd.IndexHNSWFlat if "hnsw" in tag else amd.IndexFlat)
    assert q.ntotal == nlist


@pytest.mark.parametrize("tag", TAGS)
def test_write_back_same_bytes(amd, tag, tmp_path):
    idx = amd.read_index(path(tag))
    out = tmp_path / "out.faiss"
    amd.write_index(idx, out)
    assert out.read_bytes() == open(path(tag), "rb").read()


@pytest.mark.parametrize("tag", ["sq8_l2_d72", "sqfp16_l2_d64"])
def test_mmap_and_ondisk_lists(amd, tag, tmp_path):
    """ilar read through the mmap hook, and an ilod data file, give the same lists."""
    ref = amd.read_index(path(tag))
    off, codes, ids = ref.invlists_arrays()
    mm = amd.read_index(path(tag), amd.IO_FLAG_MMAP)
    assert type(mm) is amd.IndexIVFScalarQuantizer
    o2, c2, i2 = mm.invlists_arrays()
    assert np.array_equal(off, o2) and np.array_equal(codes, c2) and np.array_equal(ids, i2)
    f, lf = tmp_path / "od.faiss", tmp_path / "od.lists"
    amd.write_index_ondisk(ref, f, lf)
    od = amd.read_index(f)
    assert type(od) is amd.IndexIVFScalarQuantizer and od.qtype == ref.qtype
    o3, c3, i3 = od.invlists_arrays()
    assert np.array_equal(off, o3) and np.array_equal(codes, c3) and np.array_equal(ids, i3)
    assert np.array_equal(od.sq_trained(), ref.sq_trained())


def test_index_factory(amd):
    a = amd.index_factory(64, "IVF32,SQ8")
    assert type(a) is amd.IndexIVFScalarQuantizer
    assert (a.qtype, a.code_size, a.nlist, a.by_residual, a.is_trained) == (QT_8bit, 64, 32, True,
                                                                          False)
    assert type(a.quantizer) is amd.IndexFlat
    b = amd.index_factory(64, "IVF32_HNSW32,SQfp16")
    assert type(b) is amd.IndexIVFScalarQuantizer
    assert (b.qtype, b.code_size, b.metric_type) == (QT_fp16, 128, amd.METRIC_L2)
    assert type(b.quantizer) is amd.IndexHNSWFlat
    c = amd.index_factory(72, "IVF16_Flat,SQ8", amd.METRIC_INNER_PRODUCT)
    assert type(c) is amd.IndexIVFScalarQuantizer
    assert (c.code_size, c.metric_type) == (72, amd.METRIC_INNER_PRODUCT)


def test_constructor_by_residual_flag(amd):
    q = amd.IndexFlatL2(16)
    a = amd.IndexIVFScalarQuantizer(q, 16, 4, QT_8bit, amd.METRIC_L2, by_residual=False)
    assert not a.by_residual and a.code_size == 16


@pytest.mark.parametrize("desc, d, needle", [
    ("IVF32,SQ4", 64, "QT_4bit"),
    ("IVF32,SQ6", 64, "QT_6bit"),
    ("IVF32,SQbf16", 64, "QT_bf16"),
    ("IVF8,SQ8", 12, "d = 12"),
    ("IVF8,SQfp16", 12, "d = 12"),
])
def test_factory_rejects(amd, desc, d, needle):
    with pytest.raises(amd.FaissError, match=needle):
        amd.index_factory(d, desc)


def test_constructor_rejects(amd):
    q = amd.IndexFlatL2(64)
    with pytest.raises(amd.FaissError, match="QT_4bit"):
        amd.IndexIVFScalarQuantizer(q, 64, 8, QT_4bit)
    q12 = amd.IndexFlatL2(12)
    with pytest.raises(amd.FaissError, match="d = 12"):
        amd.IndexIVFScalarQuantizer(q12, 12, 8, QT_8bit)


def _header(d, ntotal, trained, metric=1):
    return struct.pack("<iqqqBi", d, ntotal, 1 << 20, 1 << 20, trained, metric)


def _iwsq(d, qtype, code_size, trained):
    """An empty IwSq index laid out by hand (faiss/impl/index_write.cpp:234-241,
    367-389, 640-648): 2 lists, a flat quantizer of 2 zero centroids."""
    nlist = 2
    b = b"IwSq" + _header(d, 0, 1) + struct.pack("<QQ", nlist, 1)
    b += b"IxF2" + _header(d, nlist, 1) + struct.pack("<Q", nlist * d) + bytes(4 * nlist * d)
    b += struct.pack("<b", 0) + struct.pack("<Q", 0)  # direct map: none
    b += struct.pack("<iifQQ", qtype, 0, 0.0, d, code_size)
    b += struct.pack("<Q", len(trained)) + np.asarray(trained, np.float32).tobytes()
    b += struct.pack("<QB", code_size, 1)
    b += b"ilar" + struct.pack("<QQ", nlist, code_size) + b"sprs" + struct.pack("<Q", 0)
    return b


def test_read_rejects_other_qtypes_and_dims(amd, tmp_path):
    good = tmp_path / "good.faiss"
    good.write_bytes(_iwsq(16, QT_8bit, 16, np.ones(32)))
    idx = amd.read_index(good)  # the hand-built layout itself is readable
    assert type(idx) is amd.IndexIVFScalarQuantizer and idx.sq_trained().size == 32
    out = tmp_path / "good2.faiss"
    amd.write_index(idx, out)
    assert out.read_bytes() == good.read_bytes()
    bad = tmp_path / "q4.faiss"
    bad.write_bytes(_iwsq(16, QT_4bit, 8, np.ones(32)))
    with pytest.raises(amd.FaissError, match="QT_4bit"):
        amd.read_index(bad)
    bad.write_bytes(_iwsq(12, QT_8bit, 12, np.ones(24)))
    with pytest.raises(amd.FaissError, match="d = 12"):
        amd.read_index(bad)


def test_unsupported_operations_name_the_class(amd):
    idx = amd.read_index(path("sq8_l2_d72"))
    xq = np.zeros((2, 72), np.float32)
    with pytest.raises(amd.FaissError, match="IndexIVFScalarQuantizer"):
        idx.range_search(xq, 1.0)
    with pytest.raises(amd.FaissError, match="IndexIVFScalarQuantizer"):
        amd.clone_index(idx)
    other = amd.index_factory(72, "IVF16,SQ8")
    with pytest.raises(amd.FaissError, match="IndexIVFScalarQuantizer"):
        amd.copy_subset_to(idx, other, amd.SUBSET_TYPE_ID_MOD, 2, 0)
    with pytest.raises(amd.FaissError, match="IndexIVFScalarQuantizer"):
        amd.index_ivf_to_shards(idx, 2)
    sh = amd.IndexShardsIVF(idx.quantizer, idx.nlist)
    with pytest.raises(amd.FaissError, match="IndexIVFScalarQuantizer"):
        sh.add_shard(idx)


def test_c_symbols_exported(amd):
    names = [s for s in amd.exported_symbols() if "ScalarQuantizer" in s]
    assert len(names) == 14 and all(hasattr(amd.lib(), s) for s in names)
    assert not any(s.startswith("faiss_IndexScalarQuantizer") for s in amd.exported_symbols())


def _compile(tmp_path, name, src, *flags):
    import subprocess
    root = os.path.dirname(HERE)
    f = tmp_path / name
    f.write_text(src)
    cc = ["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
          "-I" + os.path.join(root, "include")] if name.endswith(".cpp") else \
         ["gcc", "-std=c99", "-Werror=implicit-function-declaration",
          "-I" + os.path.join(root, "include", "faiss", "c_api")]
    return subprocess.run(cc + ["-fsyntax-only", "-Wall", "-Werror", *flags, str(f)],
                          capture_output=True, text=True)


def test_c_header_declares_the_ivf_half_only(tmp_path):
    """A reference C caller keeps its include; the non-IVF IndexScalarQuantizer
    functions are absent, so their callers fail at compile time."""
    ok = _compile(tmp_path, "ok.c", """
#include "IndexScalarQuantizer_c.h"
int f(FaissIndex* q, const float* x) {
    FaissIndexIVFScalarQuantizer* ix = 0;
    if (faiss_IndexIVFScalarQuantizer_new_with_metric(&ix, q, 64, 32, QT_fp16, METRIC_L2, 1))
        return 1;
    faiss_IndexIVFScalarQuantizer_set_nprobe(ix, 4);
    faiss_IndexIVFScalarQuantizer_add_core(ix, 1, x, 0, 0);
    faiss_IndexIVFScalarQuantizer_free(faiss_IndexIVFScalarQuantizer_cast(ix));
    return (int)faiss_IndexIVFScalarQuantizer_nlist(ix);
}
""")
    assert ok.returncode == 0, ok.stderr
    bad = _compile(tmp_path, "bad.c", """
#include "IndexScalarQuantizer_c.h"
int f(void) { void* p = 0; return faiss_IndexScalarQuantizer_new(&p); }
""")
    assert bad.returncode != 0 and "faiss_IndexScalarQuantizer_new" in bad.stderr


def test_cpp_shim_headers(tmp_path):
    ok = _compile(tmp_path, "ok.cpp", """
#include <faiss/IndexScalarQuantizer.h>
#include <faiss/impl/ScalarQuantizer.h>
#include <faiss/index_factory.h>
size_t f(faiss::Index* q) {
    faiss::IndexIVFScalarQuantizer ix(q, 64, 32, faiss::ScalarQuantizer::QT_8bit,
                                      faiss::METRIC_INNER_PRODUCT, false);
    return ix.sq.code_size + ix.sq.trained.size();
}
""")
    assert ok.returncode == 0, ok.stderr
