"""tests/hnsw_params_model.py for METRIC_INNER_PRODUCT, the way the reference
does it (faiss/IndexHNSW.cpp:60-65, :337-342): the same search over the
distance -<q, y> (NegativeDistanceComputer over fvec_inner_product), every
output distance negated at the end, the (FLT_MAX, -1) padding included.

tests/test_hnsw_ip_model.py holds this to the reference-run fixtures of
scripts/make_golden_hnsw_ip.py bit for bit, stats included;
tests/test_gpu_hnsw_ip.py then uses it for shapes that have no fixture.
"""
import hashlib
import os

import numpy as np

import hnsw_params_model as hm

FLT_MAX = hm.FLT_MAX
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = {"h16": os.path.join(GOLD, "ref_hnsw_ip", "hnsw16_ip_d24.faiss"),
         "h8": os.path.join(GOLD, "ref_hnsw_ip", "hnsw8_ip_d16.faiss")}
IVF_FILES = {"ivfflat": os.path.join(GOLD, "ref_hnsw_ip", "ivf64_hnsw8_ip_flat_d32.faiss"),
             "ivfpq": os.path.join(GOLD, "ref_hnsw_ip", "ivf64_hnsw8_ip_pq8_d32.faiss")}


def load_fixtures():
    fx = dict(np.load(os.path.join(GOLD, "ref_hnsw_ip.npz")))
    fx.update(np.load(os.path.join(GOLD, "ref_hnsw_ip", "hnsw8_ip_d16.npz")))
    return fx


def jobs(fx, tag):
    """(name, k, how, ef, check, bounded, sel, nprobe) of the recorded cases."""
    out = []
    for line in fx[f"{tag}_jobs"]:
        name, k, how, ef, chk, bnd, sel, nprobe = str(line).split()
        out.append((name, int(k), how, int(ef), bool(int(chk)), bool(int(bnd)), sel, int(nprobe)))
    return out


def assert_case(fx, key, D, I, st=None):
    """D, I (and the four HNSWStats deltas) against the recorded case `key`,
    bit for bit; a k = 100 case records the sha256 of its distances."""
    np.testing.assert_array_equal(I, fx[key + "_I"], err_msg=key)
    D = np.ascontiguousarray(D, np.float32)
    if key + "_D" in fx:
        np.testing.assert_array_equal(D.view(np.uint32), fx[key + "_D"].view(np.uint32),
                                      err_msg=key)
    else:
        got = np.frombuffer(hashlib.sha256(D.tobytes()).digest(), np.uint8)
        assert np.array_equal(got, fx[key + "_Dsha"]), key + ": distances differ (sha256)"
    if st is not None:
        assert [int(v) for v in st] == [int(v) for v in fx[key + "_st"]], (key, list(st))


class NegatedIP:
    """The oracle with fvec_L2sqr(q, y) = -fvec_inner_product(q, y)."""

    def __init__(self, orc):
        self._orc = orc

    def fvec_L2sqr(self, q, y):
        return -self._orc.fvec_inner_product(q, y)

    def __getattr__(self, name):
        return getattr(self._orc, name)


class Model(hm.Model):
    def __init__(self, orc, graph):
        super().__init__(NegatedIP(orc), graph)

    def search(self, xq, k, efSearch, check_relative_distance=True, bounded_queue=True,
               member=None):
        D, I, st = super().search(xq, k, efSearch, check_relative_distance, bounded_queue, member)
        return -D, I, st  # (padding: FLT_MAX -> -FLT_MAX)
