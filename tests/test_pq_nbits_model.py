"""IndexIVFPQ with 4- to 7-bit codes, host side (no device).

tests/golden/ref_pq_nbits.npz and the index files in tests/golden/ref_pq_nbits/
were produced by the reference library (scripts/make_golden_pq_nbits.py).  The
numpy model (tests/pq_nbits_model.py) must reproduce every committed reference
result bit for bit: that pins the rule the kernels implement (packed decode,
table arithmetic, sequential code sum, strict-admission heap over (distance,
id) pairs, range rule) and the fixtures together.  Every query of every k = 10
case has a group of 8 bit-equal distances cut by the boundary, under ids that
are not in arrival order."""
import os

import numpy as np
import pytest

import pq_nbits_model as pm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "ref_pq_nbits")
TAGS = ["PQ16x4", "PQ10x5", "PQ32x6", "PQ24x7", "PQ16x4_ip"]
GEOM = {"PQ16x4": (64, 16, 4, 8), "PQ10x5": (40, 10, 5, 7), "PQ32x6": (64, 32, 6, 24),
        "PQ24x7": (96, 24, 7, 21)}


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "ref_pq_nbits.npz"))


@pytest.fixture(scope="module")
def models(amd):
    cache = {}

    def get(tag, table):
        if (tag, table) not in cache:
            idx = amd.read_index(os.path.join(GOLD, tag + ".faiss"))
            cache[(tag, table)] = pm.Model.from_index(idx, table=table)
        return cache[(tag, table)]
    return get


def cases(fx_tags=TAGS):
    out = []
    f = np.load(os.path.join(HERE, "golden", "ref_pq_nbits.npz"))
    for tag in fx_tags:
        for t in f[f"{tag}_tables"]:
            out.append((tag, max(int(t), 0)))
    return out


def test_fma_is_correctly_rounded():
    # a * b = 2^-24 (1 - 2^-46), c = 1 + 2^-23: the exact sum lies just below the
    # fp32 midpoint 1 + 2^-23 + 2^-24 and rounds down; float64 rounds it onto the
    # midpoint, from where a second rounding would go to even, 1 + 2^-22
    a = np.float32(2.0 ** -12 * (1 + 2.0 ** -23))
    b = np.float32(2.0 ** -12 * (1 - 2.0 ** -23))
    c = np.float32(1 + 2.0 ** -23)
    naive = np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    assert naive == np.float32(1 + 2.0 ** -22)
    assert pm.fma(a, b, c) == c
    # and just above the midpoint below an even neighbour
    b2 = np.float32(2.0 ** -12 * (1 + 2.0 ** -23))
    assert pm.fma(a, b2, np.float32(1)) == np.float32(1 + 2.0 ** -23)
    # exact cases and arrays
    x = np.array([1.5, -2.25, 3.0], np.float32)
    assert np.array_equal(pm.fma(x, x, np.float32(1)), x * x + 1)


def test_pack_unpack_roundtrip():
    rng = np.random.RandomState(5)
    for M, nbits in ((16, 4), (10, 5), (32, 6), (24, 7), (3, 5)):
        idx = rng.randint(0, 1 << nbits, (50, M))
        codes = pm.pack_codes(idx, nbits)
        assert codes.shape == (50, (M * nbits + 7) // 8)
        assert np.array_equal(pm.unpack_codes(codes, M, nbits), idx)
    # PQ10x5: 50 bits in 7 bytes, the top 6 bits of the last byte stay zero
    assert (pm.pack_codes(np.full((1, 10), 31), 5)[0, 6] >> 2) == 0


@pytest.mark.parametrize("tag,table", cases())
def test_model_equals_reference_search(models, fx, tag, table):
    m = models(tag, table)
    d = int(fx[f"{tag}_meta"][0])
    xq = pm_queries(fx, tag, d)
    keys, cdis = fx[f"{tag}_Iq"], fx[f"{tag}_Dq"]
    for k in fx[f"{tag}_ks"]:
        D, I = m.search_preassigned(xq, int(k), keys, cdis)
        assert np.array_equal(I, fx[f"{tag}_t{table}_{k}_I"]), (tag, table, k)
        assert np.array_equal(D, fx[f"{tag}_t{table}_{k}_D"]), (tag, table, k)


@pytest.mark.parametrize("tag,table", [("PQ16x4", 1), ("PQ16x4", 0), ("PQ16x4_ip", 0)])
def test_model_equals_reference_range(models, fx, tag, table):
    m = models(tag, table)
    xq = pm_queries(fx, tag, int(fx[f"{tag}_meta"][0]))
    tt = f"{tag}_t{table}"
    lims, D, I = m.range_search_preassigned(xq, fx[f"{tt}_radius"], fx[f"{tag}_Iq"],
                                            fx[f"{tag}_Dq"])
    assert np.array_equal(lims, fx[f"{tt}_range_lims"])
    assert np.array_equal(I, fx[f"{tt}_range_I"])
    assert np.array_equal(D, fx[f"{tt}_range_D"])


@pytest.mark.parametrize("table", [1, 0])
def test_model_equals_reference_max_codes_selector(models, fx, table):
    m = models("PQ16x4", table)
    xq = pm_queries(fx, "PQ16x4", 64)
    sel = set(range(0, 2000, 3))
    D, I = m.search_preassigned(xq, 10, fx["PQ16x4_Iq"], fx["PQ16x4_Dq"], sel=sel,
                                max_codes=150)
    assert np.array_equal(I, fx[f"PQ16x4_t{table}_params_I"])
    assert np.array_equal(D, fx[f"PQ16x4_t{table}_params_D"])


def pm_queries(fx, tag, d):
    """The case's queries: the ref_float_rand stream of seed + 2 (oracle.float_rand
    is the same generator)."""
    import __graft_entry__ as ge
    seed = int(fx[f"{tag}_meta"][6])
    return ge.load_oracle().float_rand(32 * d, seed + 2).reshape(32, d)


def test_boundary_ties_in_every_query(fx):
    for tag, table in cases():
        D = fx[f"{tag}_t{table}_10_D"]
        for row in D:
            assert 0 < (row == row[9]).sum() < 8, (tag, table)


@pytest.mark.parametrize("tag", sorted(GEOM))
def test_factory_code_size(amd, tag):
    d, M, nbits, cs = GEOM[tag]
    for desc in (f"IVF16,{tag}", f"IVF16,{tag}np"):
        idx = amd.index_factory(d, desc)
        assert type(idx) is amd.IndexIVFPQ
        assert idx.code_size == cs
        info = idx.pq_info()
        assert (info["M"], info["nbits"]) == (M, nbits)
        assert idx.pq_centroids.shape == (M, 1 << nbits, d // M)
    rf = amd.index_factory(d, f"IVF16,{tag},RFlat")
    assert type(rf) is amd.IndexRefineFlat and rf.base_index.code_size == cs


@pytest.mark.parametrize("tag", TAGS)
def test_read_write_roundtrip(amd, fx, tag, tmp_path):
    src = os.path.join(GOLD, tag + ".faiss")
    idx = amd.read_index(src)
    d, nlist, nb, ml2, _, _, _, M, nbits = (int(v) for v in fx[f"{tag}_meta"][:9])
    assert (idx.d, idx.nlist, idx.ntotal) == (d, nlist, nb)
    assert idx.code_size == (M * nbits + 7) // 8 and idx.pq_info()["nbits"] == nbits
    # the lists as the reference holds them
    sizes = fx[f"{tag}_list_sizes"]
    off = np.concatenate([[0], np.cumsum(sizes)])
    for l in range(nlist):
        assert np.array_equal(idx.list_codes(l), fx[f"{tag}_list_codes"][off[l]:off[l + 1]])
        assert np.array_equal(idx.list_ids(l), fx[f"{tag}_list_ids"][off[l]:off[l + 1]])
    out = tmp_path / "back.faiss"
    amd.write_index(idx, out)
    assert open(out, "rb").read() == open(src, "rb").read()
    clone = amd.clone_index(idx)
    out2 = tmp_path / "clone.faiss"
    amd.write_index(clone, out2)
    assert open(out2, "rb").read() == open(src, "rb").read()


@pytest.mark.parametrize("nbits", [3, 9, 16])
def test_unserved_widths_raise(amd, nbits):
    q = amd.IndexFlatL2(64)
    with pytest.raises(amd.FaissError, match=rf"nbits = {nbits}\b"):
        amd.IndexIVFPQ(q, 64, 16, 16, nbits)
    with pytest.raises(amd.FaissError, match="nbits"):
        amd.index_factory(64, f"IVF16,PQ16x{nbits}")
