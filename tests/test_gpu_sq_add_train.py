"""IndexIVFScalarQuantizer add and train against reference runs
(tests/golden/ref_sq*, scripts/make_golden_sq.py).

The training, base and add sets are float_rand streams recorded as (rows, d,
seed) with the SHA-256 of the bytes the reference consumed; the library's
float_rand restates the stream, and the digest is checked before use."""
import hashlib
import os

import numpy as np
import pytest

from conftest import assert_same_results

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FACTORY = {
    "sq8_l2_d64": "IVF32,SQ8",
    "sq8_l2_d72": "IVF16,SQ8",
    "sqfp16_l2_d64": "IVF32,SQfp16",
    "sq8_ip_d64": "IVF32,SQ8",
    "sq8_hnsw_d64": "IVF32_HNSW32,SQ8",
}
TAGS = list(FACTORY)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "ref_sq.npz"))


def read(amd, tag):
    return amd.read_index(os.path.join(HERE, "golden", "ref_sq", tag + ".faiss"))


def stream(amd, fx, tag, what):
    """The recorded input set `what` (xt / xb / xa) of a tag, digest checked."""
    d, _, nb, nt, _, _, s_xt, s_xb, _, s_xa, na = (int(v) for v in fx[f"{tag}_meta"])
    n, seed = {"xt": (nt, s_xt), "xb": (nb, s_xb), "xa": (na, s_xa)}[what]
    x = amd.float_rand(n * d, seed).reshape(n, d)
    if what == "xb":  # the last 10 % are copies of the first rows
        x[nb - nb // 10:] = x[:nb // 10]
    got = np.frombuffer(hashlib.sha256(x.tobytes()).digest(), np.uint8)
    assert np.array_equal(got, fx[f"{tag}_{what}_sha"]), f"{tag} {what}: not the recorded input"
    return x


@pytest.mark.parametrize("tag", TAGS)
def test_add_lists_and_codes(amd, gpu, fx, tag):
    idx = read(amd, tag)
    nlist, nb = idx.nlist, idx.ntotal
    xa = stream(amd, fx, tag, "xa")
    la, codes = fx[f"{tag}_xa_assign"].astype(np.int64), fx[f"{tag}_xa_codes"]
    before = [idx.get_list_size(l) for l in range(nlist)]
    idx.add(xa)
    assert idx.ntotal == nb + len(xa)
    for l in range(nlist):
        mine = np.nonzero(la == l)[0]
        assert idx.get_list_size(l) == before[l] + mine.size
        assert np.array_equal(idx.list_ids(l)[before[l]:], nb + mine)
        assert np.array_equal(idx.list_codes(l)[before[l]:], codes[mine])


@pytest.mark.parametrize("tag", TAGS)
def test_train_add_search(amd, gpu, fx, tag):
    ref = read(amd, tag)
    d, nlist, nb, _, ml2 = (int(v) for v in fx[f"{tag}_meta"][:5])
    q = ref.quantizer
    cent = q.storage_vectors() if "hnsw" in tag else q.xb
    assert cent.shape == (nlist, d)
    idx = amd.index_factory(d, FACTORY[tag], amd.METRIC_L2 if ml2 else amd.METRIC_INNER_PRODUCT)
    idx.quantizer.add(cent)  # train() then skips k-means
    assert not idx.is_trained
    idx.train(stream(amd, fx, tag, "xt"))
    assert idx.is_trained
    tr, tr_ref = idx.sq_trained(), ref.sq_trained()
    assert tr.size == tr_ref.size
    assert np.array_equal(tr.view(np.uint32), tr_ref.view(np.uint32))
    idx.add_with_ids(stream(amd, fx, tag, "xb"), np.arange(nb, dtype=np.int64) * 3 + 7)
    for l in range(nlist):
        assert np.array_equal(idx.list_ids(l), ref.list_ids(l))
        assert np.array_equal(idx.list_codes(l), ref.list_codes(l))
    xq = fx[f"{tag}_xq"]
    idx.nprobe = 4
    D, I = idx.search_preassigned(xq, 10, fx[f"{tag}_q4_I"].astype(np.int64), fx[f"{tag}_q4_D"])
    assert_same_results(D, I, fx[f"{tag}_pre_4_10_D"], fx[f"{tag}_pre_4_10_I"].astype(np.int64))
    D, I = idx.search(xq, 10)
    assert_same_results(D, I, fx[f"{tag}_full_4_10_D"], fx[f"{tag}_full_4_10_I"].astype(np.int64))
