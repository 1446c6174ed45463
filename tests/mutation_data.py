"""The reference-run mutation fixtures (scripts/make_golden_mutation.py):
tests/golden/ref_mutation.npz, tests/golden/ref_mutation/<tag>.npz and
tests/golden/ref_mutation/*.faiss, and the
helpers both test files share.  A missing fixture is an error, never a skip."""
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "ref_mutation")
TAGS = ["flat", "pq8", "pq12x5", "sq8", "sqfp16"]
REMOVALS = ["range", "batch", "array"]
_fx = None


def fixtures():
    global _fx
    if _fx is None:
        _fx = dict(np.load(os.path.join(HERE, "golden", "ref_mutation.npz")))
        for tag in TAGS:  # one file per index, keys <tag>_<record>
            _fx.update(np.load(os.path.join(GOLD, tag + ".npz")))
    return _fx


def path(name):
    fn = os.path.join(GOLD, name + ".faiss")
    assert os.path.exists(fn), f"fixture {fn} is missing (scripts/make_golden_mutation.py)"
    return fn


def text(a):
    return bytes(a).decode().rstrip("\0")  # (the reference's msg keeps its buffer's NUL)


def selector(amd, fx, tag, how):
    ids = fx[f"{tag}_rm_{how}_sel"]
    if how == "range":
        return amd.IDSelectorRange(int(ids[0]), int(ids[1]))
    if how == "batch":
        return amd.IDSelectorBatch(ids)
    return amd.IDSelectorArray(ids)  # array, hash


def assert_lists(idx, fx, prefix):
    """The lists of idx equal the recorded sizes, ids (in order) and codes."""
    sizes = fx[prefix + "_sizes"]
    ids = fx[prefix + "_ids"]
    sha = fx[prefix + "_codes_sha"]
    assert idx.nlist == len(sizes)
    p = 0
    for l, n in enumerate(sizes):
        assert idx.get_list_size(l) == n, (prefix, l)
        got = idx.list_ids(l)
        assert np.array_equal(got, ids[p:p + n]), \
            f"{prefix}: list {l} holds {got[:8]}..., the reference {ids[p:p + 8]}..."
        h = np.frombuffer(hashlib.sha256(idx.list_codes(l).tobytes()).digest(), np.uint8)
        assert np.array_equal(h, sha[l]), f"{prefix}: codes of list {l} differ"
        p += n
    assert idx.ntotal == p


def map_pairs(idx, ids):
    """[(id, lo)] of idx's direct map for the given ids (absent ids left out)."""
    out = []
    for i in ids:
        try:
            l, o = idx.direct_map_get(int(i))
        except Exception:
            continue
        out.append((int(i), (l << 32) | o))
    return np.array(out, np.int64).reshape(-1, 2)
