"""tests/hnsw_params_model.py (a plain Python restatement of HNSW::search's
three level-0 modes and the result selector) against the reference-run
fixtures of scripts/make_golden_hnsw_params.py: D, I and the four HNSWStats
deltas of every standalone case, bit for bit.  No GPU: this pins the model
that tests/test_gpu_hnsw_params.py uses for shapes without a fixture.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hnsw_params_model as hm  # noqa: E402

FX = np.load(os.path.join(HERE, "golden", "ref_hnsw_params.npz"))
FILES = {"dup": os.path.join(HERE, "golden", "ref_full", "hnsw_dup.faiss"),
         "h24": os.path.join(HERE, "golden", "ref_hnsw_params", "hnsw16_d24.faiss")}


def jobs(tag):
    """(name, k, how, ef, check, bounded, sel, nprobe) of the packed cases."""
    out = []
    for line in FX[f"{tag}_jobs"]:
        name, k, how, ef, chk, bnd, sel, nprobe = str(line).split()
        out.append((name, int(k), how, int(ef), bool(int(chk)), bool(int(bnd)), sel, int(nprobe)))
    return out


def member_of(sel, n):
    """The driver's selector spec over ids 0 .. n - 1 as a bool array."""
    if sel == "none":
        return None
    p = sel.split(":")
    ids = np.arange(n)
    if p[0] == "range":
        return (ids >= int(p[1])) & (ids < int(p[2]))
    m = np.isin(ids, int(p[1]) + int(p[2]) * np.arange(int(p[3])))
    return ~m if p[0] == "notbatch" else m


def resolved(job):
    """(efSearch, check, bounded, sel) a case runs with: how = index sets the
    values on the index, how = cleared passes default-constructed params."""
    name, k, how, ef, chk, bnd, sel, _ = job
    if how == "cleared":
        return 16, True, True, "none"
    return ef, chk, bnd, sel


@pytest.fixture(scope="module")
def models(amd, orc):
    out = {}
    for tag, fn in FILES.items():
        out[tag] = hm.Model(orc, orc.HNSWGraph.from_index(amd.read_index(fn)))
    return out


@pytest.mark.parametrize("tag", ["dup", "h24"])
def test_model_equals_reference(models, tag):
    m = models[tag]
    xq = FX[f"{tag}_xq"]
    js = jobs(tag)
    assert len(js) >= 40
    for job in js:
        name, k = job[0], job[1]
        ef, chk, bnd, sel = resolved(job)
        D, I, st = m.search(xq, k, ef, chk, bnd, member_of(sel, m.ntotal))
        np.testing.assert_array_equal(I, FX[f"{tag}_{name}_I"], err_msg=name)
        np.testing.assert_array_equal(D, FX[f"{tag}_{name}_D"], err_msg=name)
        np.testing.assert_array_equal(st, FX[f"{tag}_{name}_st"], err_msg=name)
