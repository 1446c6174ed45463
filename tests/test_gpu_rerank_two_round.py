"""The IVF-Flat re-rank's two-round evaluation (ivf_rerank.h k_ivf_rerank: a
first exact pass over the P = 16 ceil(k / 16) candidates with the smallest
upper bounds, then only the candidates whose lower bound is <= the k-th exact
key of that pass) against the oracle, bit for bit: both values of P, ties at
the threshold and at the k boundary (the arrival-order resolve), fewer
candidates than k, inner product, the KT = 8 instantiation, and a query whose
failing stream takes the single-sweep path.
"""
import re

import numpy as np
import pytest

from conftest import assert_same_results, rand

pytestmark = pytest.mark.gpu

D64, NB, NLIST, NPROBE, NQ = 64, 20000, 64, 8, 256


def make(amd, desc, xb, nprobe, train=None, metric=None):
    idx = (amd.index_factory(xb.shape[1], desc) if metric is None
           else amd.index_factory(xb.shape[1], desc, metric))
    idx.train(xb if train is None else train)
    idx.add(xb)
    idx.nprobe = nprobe
    return idx


def same_as_oracle(orc, idx, xq, k, nprobe):
    D, I = idx.search(xq, k)
    Dr, Ir, _, _ = orc.IVFOracle.from_index(idx).search(xq, k, nprobe, nslices=1)
    assert_same_results(D, I, Dr, Ir)
    return D, I


@pytest.fixture(scope="module")
def base(orc):
    return rand(orc, NB, D64, 4101), rand(orc, NQ, D64, 4102)


@pytest.fixture(scope="module")
def index(amd, gpu, base):
    return make(amd, f"IVF{NLIST},Flat", base[0], NPROBE)


@pytest.fixture(scope="module")
def index_x25(amd, gpu, base):
    # every base vector 25 times: each query's k-th distance is shared
    xb = base[0]
    return make(amd, f"IVF{NLIST},Flat", np.ascontiguousarray(np.tile(xb, (25, 1))), NPROBE,
                train=xb)


@pytest.mark.parametrize("k", [1, 10, 16, 17, 32])
def test_both_round_sizes(amd, orc, gpu, base, index, k):
    same_as_oracle(orc, index, base[1], k, NPROBE)


@pytest.mark.parametrize("k", [1, 10, 16, 17, 32])
def test_ties_at_threshold_and_boundary(amd, orc, gpu, base, index_x25, k):
    D, I = same_as_oracle(orc, index_x25, base[1], k, NPROBE)
    if k > 1:  # 25 copies: the first k results of a query share distances
        assert (D[:, 0] == D[:, 1]).all()


def test_fewer_candidates_than_k(amd, orc, gpu):
    xb, xq = rand(orc, 50, D64, 4103), rand(orc, 64, D64, 4104)
    idx = make(amd, "IVF8,Flat", xb, 2)
    D, I = same_as_oracle(orc, idx, xq, 10, 2)
    assert (I == -1).any()  # some query's two lists hold fewer than 10 rows


def test_identical_vectors(amd, orc, gpu):
    xb = np.ascontiguousarray(np.tile(rand(orc, 1, D64, 4105), (3000, 1)))
    xq = rand(orc, 64, D64, 4106)
    idx = make(amd, "IVF8,Flat", xb, 2, train=rand(orc, 400, D64, 4107))
    same_as_oracle(orc, idx, xq, 10, 2)


@pytest.mark.parametrize("k", [10, 32])
def test_inner_product_d30(amd, orc, gpu, k):
    xb, xq = rand(orc, NB, 30, 4108), rand(orc, NQ, 30, 4109)
    idx = make(amd, f"IVF{NLIST},Flat", xb, NPROBE, metric=amd.METRIC_INNER_PRODUCT)
    same_as_oracle(orc, idx, xq, k, NPROBE)


@pytest.mark.parametrize("k", [10, 32])
def test_long_lists_kt8(amd, orc, gpu, k):
    # 40 000 / 64 = 625 rows per list on average (>= 512): 8 kept keys per stream
    xb, xq = rand(orc, 40000, D64, 4110), rand(orc, NQ, D64, 4111)
    idx = make(amd, f"IVF{NLIST},Flat", xb, 16)
    same_as_oracle(orc, idx, xq, k, 16)


def test_failing_stream_takes_single_sweep(amd, orc, gpu, monkeypatch, capfd):
    # one list holds 40 copies of a vector next to the queries: with k = 32 a
    # stream keeps fewer keys than it has rows under U, so it fails and the
    # query goes through the unchanged path
    xb = rand(orc, NB, D64, 4112).copy()
    xq = rand(orc, 64, D64, 4113)
    c = xq.mean(axis=0)
    xb[100:140] = c
    xq = np.ascontiguousarray(c + 0.01 * (xq - c))
    idx = make(amd, f"IVF{NLIST},Flat", xb, NPROBE)
    monkeypatch.setenv("FAISS_AMD_IVF_STATS", "1")
    capfd.readouterr()
    same_as_oracle(orc, idx, xq, 32, NPROBE)
    err = capfd.readouterr().err
    m = re.findall(r"ivf mfma scan: .*failing probes/q=([0-9.]+)", err)
    assert m, err
    assert float(m[-1]) > 0.0, err


def test_exact_rows_counter(amd, orc, gpu, base, index, monkeypatch, capfd):
    k = 10
    monkeypatch.setenv("FAISS_AMD_IVF_STATS", "1")
    capfd.readouterr()
    same_as_oracle(orc, index, base[1], k, NPROBE)
    err = capfd.readouterr().err
    m = re.findall(r"ivf mfma scan: .*survivors/q=([0-9.]+) exact rows/q=([0-9.]+)", err)
    assert m, err
    surv, rows = float(m[-1][0]), float(m[-1][1])
    print(f"survivors/q={surv} exact rows/q={rows}")
    assert k <= rows <= surv, err
