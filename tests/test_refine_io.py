"""IndexRefineFlat on the host side: index_factory builds it (",RFlat" /
",Refine(Flat)"), the reference's IxRF files (tests/golden/ref_refine, written
by the reference's write_index through scripts/make_golden_refine.py) read,
describe themselves, write back and clone byte for byte, ParameterSpace reaches
the wrapper and its base index, and a C caller of the reference's
c_api/IndexFlat_c.h compiles and links.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "ref_refine")
TAGS = ["pq_l2_d64", "pq_l2_d64_kf25", "pq_l2_d64_np1", "flat_ip_d40", "flat_ip_d44",
        "sq8_l2_d72", "pq_l2_d96_k1", "sq8_ip_d40"]
BASE = {"pq": "IndexIVFPQ", "flat": "IndexIVFFlat", "sq8": "IndexIVFScalarQuantizer"}


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "ref_refine.npz"))


def path(tag):
    return os.path.join(GOLD, tag + ".faiss")


def test_every_committed_file_is_a_case(amd):
    files = sorted(f for f in os.listdir(GOLD) if f.endswith(".faiss"))
    assert [f[:-6] for f in files] == sorted(TAGS)
    for f in files:
        assert type(amd.read_index(os.path.join(GOLD, f))) is amd.IndexRefineFlat


@pytest.mark.parametrize("desc, d, base, metric", [
    ("IVF32,PQ8,RFlat", 64, "IndexIVFPQ", "l2"),
    ("IVF16,Flat,Refine(Flat)", 40, "IndexIVFFlat", "ip"),
    ("HNSW32,RFlat", 32, "IndexHNSWFlat", "l2"),
    ("Flat,RFlat", 12, "IndexFlat", "ip"),
    ("IVF16_HNSW32,SQ8,RFlat", 72, "IndexIVFScalarQuantizer", "l2"),
])
def test_index_factory(amd, desc, d, base, metric):
    m = amd.METRIC_L2 if metric == "l2" else amd.METRIC_INNER_PRODUCT
    idx = amd.index_factory(d, desc, m)
    assert type(idx) is amd.IndexRefineFlat
    assert idx.k_factor == 1.0 and idx.own_fields
    assert (idx.d, idx.metric_type, idx.ntotal) == (d, m, 0)
    b, r = idx.base_index, idx.refine_index
    assert type(b).__name__ == base and type(r) is amd.IndexFlat
    assert (b.d, b.metric_type, r.d, r.metric_type) == (d, m, d, m)
    assert idx.is_trained == b.is_trained


def test_factory_rejects_other_refine_types(amd):
    with pytest.raises(amd.FaissError, match="refine index of type PQ8 is not served"):
        amd.index_factory(64, "IVF32,PQ8,Refine(PQ8)")
    # the suffix is taken off before the base description is judged
    with pytest.raises(amd.FaissError, match=r"unsupported index_factory string LSH$"):
        amd.index_factory(64, "LSH,RFlat")
    with pytest.raises(amd.FaissError, match=r"unsupported index_factory string LSH$"):
        amd.index_factory(64, "LSH,Refine(Flat)")


@pytest.mark.parametrize("tag", TAGS)
def test_read_describe(amd, fx, tag):
    d, nlist, nb, ml2, nprobe = (int(v) for v in fx[f"{tag}_meta"][:5])
    idx = amd.read_index(path(tag))
    assert type(idx) is amd.IndexRefineFlat
    assert idx.k_factor == float(fx[f"{tag}_k_factor"])
    assert idx.own_fields and idx.is_trained
    m = amd.METRIC_L2 if ml2 else amd.METRIC_INNER_PRODUCT
    assert (idx.d, idx.ntotal, idx.metric_type) == (d, nb, m)
    b, r = idx.base_index, idx.refine_index
    assert type(b).__name__ == BASE[tag.split("_")[0]]
    assert (b.nlist, b.nprobe, b.ntotal, b.d) == (nlist, nprobe, nb, d)
    assert type(r) is amd.IndexFlat and (r.ntotal, r.d, r.metric_type) == (nb, d, m)
    # ids are rows of the flat storage
    ids = np.concatenate([b.list_ids(l) for l in range(nlist)])
    assert np.array_equal(np.sort(ids), np.arange(nb))
    assert r.xb.shape == (nb, d)


@pytest.mark.parametrize("tag", TAGS)
def test_write_back_same_bytes(amd, tag, tmp_path):
    idx = amd.read_index(path(tag))
    out = tmp_path / "out.faiss"
    amd.write_index(idx, out)
    assert out.read_bytes() == open(path(tag), "rb").read()


@pytest.mark.parametrize("tag", TAGS)
def test_clone_same_bytes(amd, tag, tmp_path):
    idx = amd.read_index(path(tag))
    cl = amd.clone_index(idx)
    assert type(cl) is amd.IndexRefineFlat and cl.k_factor == idx.k_factor
    del idx
    out = tmp_path / "clone.faiss"
    amd.write_index(cl, out)
    assert out.read_bytes() == open(path(tag), "rb").read()


def test_planted_pairs_tie_and_separate_the_tie_rules(amd, fx):
    """What the fixtures must hold to catch a (distance, id) sort: the planted
    rows tie bit for bit, and the reference's k = 1 result is the larger id for
    at least two queries per case.  Where the base distances are approximate
    (PQ, SQ8) the pair's base order is not its id order, so at least two
    queries return the smaller id as well: neither id direction passes.  (With
    an IVF-Flat base the pair ties in the base row too and arrives larger id
    first, so those cases pin the inner-product direction only.)"""
    for tag, ml2, approx in (("pq_l2_d64", 1, True), ("flat_ip_d40", 0, False),
                             ("flat_ip_d44", 0, False), ("sq8_ip_d40", 0, True)):
        xb = amd.read_index(path(tag)).refine_index.xb.astype(np.float64)
        xq = fx[f"{tag}_xq"].astype(np.float64)
        pairs, I1 = fx[f"{tag}_pairs"], fx[f"{tag}_1_I"]
        assert len(pairs) == 8
        larger = 0
        for j, plus, minus in pairs:
            if ml2:
                a, b = ((xq[j] - xb[plus]) ** 2).sum(), ((xq[j] - xb[minus]) ** 2).sum()
            else:
                a, b = (xq[j] * xb[plus]).sum(), (xq[j] * xb[minus]).sum()
            assert a == b and a == np.float32(a)  # exact in fp32, in any order
            assert I1[j, 0] in (plus, minus)
            larger += int(I1[j, 0] == max(plus, minus))
        assert larger >= 2
        if approx:
            assert larger <= 6  # ... and neither is it "the larger id"


def test_parameter_space(amd):
    idx = amd.read_index(path("pq_l2_d64"))
    ps = amd.ParameterSpace()
    ps.set_index_parameter(idx, "k_factor_rf", 7)
    assert idx.k_factor == 7.0
    ps.set_index_parameter(idx, "k_factor_rf", 2.9)  # int(val), faiss/AutoTune.cpp:483-491
    assert idx.k_factor == 2.0
    ps.set_index_parameter(idx, "nprobe", 9)
    assert idx.base_index.nprobe == 9
    h = amd.index_factory(16, "HNSW16,RFlat")
    ps.set_index_parameter(h, "efSearch", 77)
    assert h.base_index.efSearch == 77
    with pytest.raises(amd.FaissError, match="unknown parameter"):
        ps.set_index_parameter(idx, "no_such_parameter", 1)


def test_host_side_members(amd):
    rng = np.random.RandomState(3)
    x = rng.rand(40, 8).astype(np.float32)
    base = amd.IndexFlatL2(8)
    idx = amd.IndexRefineFlat(base)
    assert not idx.own_fields and idx.k_factor == 1.0 and idx.is_trained
    idx.add(x[:25])
    idx.add(x[25:])
    assert (idx.ntotal, base.ntotal, idx.refine_index.ntotal) == (40, 40, 40)
    assert np.array_equal(idx.refine_index.xb, x)
    with pytest.raises(amd.FaissError, match="add_with_ids"):
        idx.add_with_ids(x[:2], np.arange(2))
    idx.reset()
    assert (idx.ntotal, base.ntotal, idx.refine_index.ntotal) == (0, 0, 0)
    base.add(x)
    # a populated base: the reference's IndexRefine constructor already throws
    # on the ntotal mismatch with the new, empty storage
    with pytest.raises(amd.FaissError, match="ntotal"):
        amd.IndexRefineFlat(base)


def test_c_symbols_exported(amd):
    names = [s for s in amd.exported_symbols() if "Refine" in s]
    assert sorted(names) == sorted(
        ["faiss_IndexRefineFlat_" + s for s in ("new", "free", "cast", "own_fields",
                                                 "set_own_fields", "k_factor", "set_k_factor")] +
        ["faiss_amd_IndexRefine_base_index", "faiss_amd_IndexRefine_refine_index",
         "faiss_amd_IndexRefineSearchParameters_new",
         "faiss_amd_IndexRefineSearchParameters_free"])
    assert all(hasattr(amd.lib(), s) for s in names)


C_PROGRAM = """
#include <stdio.h>
#include <faiss/c_api/IndexFlat_c.h>
int main(void) {
    FaissIndexFlat* base = 0;
    FaissIndexRefineFlat* rf = 0;
    if (faiss_IndexFlat_new_with(&base, 16, METRIC_L2)) return 1;
    if (faiss_IndexRefineFlat_new(&rf, base)) return 2;
    if (!faiss_IndexRefineFlat_cast(rf) || faiss_IndexRefineFlat_cast(base)) return 3;
    if (faiss_IndexRefineFlat_k_factor(rf) != 1.0f || faiss_IndexRefineFlat_own_fields(rf)) return 4;
    faiss_IndexRefineFlat_set_k_factor(rf, 2.5f);
    if (faiss_IndexRefineFlat_k_factor(rf) != 2.5f) return 5;
    if (faiss_Index_d(rf) != 16 || faiss_Index_ntotal(rf) != 0) return 6;
    faiss_IndexRefineFlat_free(rf);
    faiss_IndexFlat_free(base);
    printf("ok\\n");
    return 0;
}
"""


def test_c_program_compiles_links_and_runs(amd, tmp_path):
    """A caller of the reference's IndexRefineFlat C API: strict C99 against
    <faiss/c_api/IndexFlat_c.h>, linked with the library, run without a GPU."""
    src = tmp_path / "rf.c"
    src.write_text(C_PROGRAM)
    exe = tmp_path / "rf"
    libdir = os.path.dirname(amd.LIB_PATH)
    cc = subprocess.run(
        ["gcc", "-std=c99", "-Wall", "-Werror", "-Werror=implicit-function-declaration",
         "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L" + libdir,
         "-lfaiss_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"],
        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stderr)


def test_cpp_shim_header(tmp_path):
    src = tmp_path / "ok.cpp"
    src.write_text("""
#include <faiss/IndexRefine.h>
#include <faiss/IndexFlat.h>
float f(faiss::Index* base, const float* xb) {
    faiss::IndexRefineFlat a(base), b(base, xb);
    faiss::IndexRefineSearchParameters p;
    p.k_factor = 4;
    p.base_index_params = nullptr;
    faiss::IndexRefine* r = &a;
    return r->k_factor + (r->own_fields ? 1 : 0) + (r->refine_index == b.refine_index);
}
""")
    cc = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                         "-I" + os.path.join(ROOT, "include"), "-fsyntax-only", "-Wall", "-Werror",
                         str(src)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
