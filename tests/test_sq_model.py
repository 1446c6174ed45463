"""The numpy model of the IVF-SQ search (tests/sq_model.py) against every
recorded reference run, host side (no device).

  * tests/golden/ref_sq*: five indexes the reference trained and filled
    (scripts/make_golden_sq.py): search_preassigned at nprobe 1 / 4 / nlist and
    k 1 / 10 / 100, the all-rows result, store_pairs, max_codes with a selector,
    and encode_vectors;
  * the four IVF-SQ indexes of tests/golden/ref_hard (signed and offset data);
  * tests/golden/ref_sq_edges* (scripts/make_golden_sq_edges.py): hand-laid
    indexes with by_residual off and on, SQfp16 with inner product, d = 8, 24,
    72 and 264, lists of 0, 1, 255, 256, 257 and 513 rows, clamped codes, a
    vdiff == 0 dimension, +-inf / NaN / subnormal / -0.0 halves, probes in
    order, reversed, with a -1 and with a list named twice, ties at the k-th
    place, k beyond the admitted rows.
Everything is bit for bit.  That pins the rule csrc/kernels_sq.hip implements
and the model test_gpu_sq_edges.py compares the kernel with at other shapes.
The reference's own answers on non-finite distances are pinned too: an L2 row at
+inf or NaN is never admitted and the result is padded; an inner-product row at
+inf is returned, the first arrival winning a tie at the k-th place; -inf and
NaN inner products are never admitted."""
import hashlib
import os

import numpy as np
import pytest

import sq_edges_data as sd
import sq_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
SQ_TAGS = ["sq8_l2_d64", "sq8_l2_d72", "sqfp16_l2_d64", "sq8_ip_d64", "sq8_hnsw_d64"]
PAIR_TAGS = ["sq8_l2_d64", "sq8_ip_d64"]
HARD_TAGS = ["sq8_signed", "sq8_offset4", "sqfp16_signed", "sqfp16_offset4"]


def same(D, I, Dr, Ir, what):
    """ids equal and distances equal as bit patterns (NaN included)"""
    assert D.shape == Dr.shape and I.shape == Ir.shape, what
    np.testing.assert_array_equal(I, Ir.astype(np.int64), err_msg=str(what))
    np.testing.assert_array_equal(D.view(np.uint32), Dr.view(np.uint32), err_msg=str(what))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "ref_sq.npz"))


@pytest.fixture(scope="module")
def ex():
    return np.load(os.path.join(GOLD, "ref_sq_edges.npz"))


@pytest.fixture(scope="module")
def models(amd):
    cache = {}

    def get(folder, tag):
        if (folder, tag) not in cache:
            idx = amd.read_index(os.path.join(GOLD, folder, tag + ".faiss"))
            cache[(folder, tag)] = sm.Model.from_index(idx)
        return cache[(folder, tag)]
    return get


# ---------------------------------------------------------------- ref_sq
@pytest.mark.parametrize("tag", SQ_TAGS)
def test_ref_sq_search_preassigned(models, fx, tag):
    m = models("ref_sq", tag)
    xq = fx[f"{tag}_xq"]
    n = 0
    for key in fx.files:
        if not (key.startswith(tag + "_pre_") and key.endswith("_D")):
            continue
        nprobe, k = (int(v) for v in key[len(tag) + 5:-2].split("_"))
        D, I = m.search_preassigned(xq, k, fx[f"{tag}_q{nprobe}_I"], fx[f"{tag}_q{nprobe}_D"])
        same(D, I, fx[key], fx[key[:-2] + "_I"], key)
        n += 1
    assert n == 9


def test_ref_sq_all_rows(models, fx):
    tag = "sq8_l2_d72"
    m = models("ref_sq", tag)
    Dr, Ir = fx[f"{tag}_all_D"], fx[f"{tag}_all_I"]
    nq, nb = Dr.shape
    nlist = int(fx[f"{tag}_meta"][1])
    D, I = m.search_preassigned(fx[f"{tag}_xq"][:nq], nb, fx[f"{tag}_q{nlist}_I"][:nq],
                                fx[f"{tag}_q{nlist}_D"][:nq])
    same(D, I, Dr, Ir, tag)


@pytest.mark.parametrize("tag", PAIR_TAGS)
def test_ref_sq_store_pairs_and_params(models, fx, tag):
    m = models("ref_sq", tag)
    xq = fx[f"{tag}_xq"]
    D, I = m.search_preassigned(xq, 10, fx[f"{tag}_q4_I"], fx[f"{tag}_q4_D"], store_pairs=True)
    same(D, I, fx[f"{tag}_sp_D"], fx[f"{tag}_sp_I"], "sp")
    # IndexIVF::search with nprobe = 8: the first eight probes of the 32 recorded
    nb = int(fx[f"{tag}_meta"][2])
    sel = set((np.arange(nb, dtype=np.int64) * 3 + 7)[::2].tolist())
    D, I = m.search_preassigned(xq, 10, fx[f"{tag}_q32_I"][:, :8], fx[f"{tag}_q32_D"][:, :8],
                                sel=sel, max_codes=300)
    same(D, I, fx[f"{tag}_params_D"], fx[f"{tag}_params_I"], "params")


@pytest.mark.parametrize("tag", SQ_TAGS)
def test_ref_sq_encode(models, orc, fx, tag):
    m = models("ref_sq", tag)
    d, na, seed = int(fx[f"{tag}_meta"][0]), int(fx[f"{tag}_meta"][10]), int(fx[f"{tag}_meta"][9])
    xa = orc.float_rand(na * d, seed).reshape(na, d)
    got = np.frombuffer(hashlib.sha256(xa.tobytes()).digest(), np.uint8)
    assert np.array_equal(got, fx[f"{tag}_xa_sha"]), "not the recorded input"
    np.testing.assert_array_equal(m.encode(xa, fx[f"{tag}_xa_assign"]), fx[f"{tag}_xa_codes"])


# ---------------------------------------------------------------- ref_hard
@pytest.mark.parametrize("tag", HARD_TAGS)
def test_ref_hard_search_preassigned(models, tag):
    m = models("ref_hard", tag)
    res = np.load(os.path.join(GOLD, "ref_hard", tag + ".npz"))
    xq = np.load(os.path.join(GOLD, "ref_hard.npz"))[tag.split("_")[1] + "_d64_xq"]
    n = 0
    for nprobe in (4, 8):
        for k in (1, 10, 100):
            key = f"pre_{nprobe}_{k}"
            D, I = m.search_preassigned(xq, k, res[f"q{nprobe}_I"], res[f"q{nprobe}_D"])
            same(D, I, res[key + "_D"], res[key + "_I"], key)
            n += 1
    assert n == len([f for f in res.files if f.startswith("pre_") and f.endswith("_D")])


# ---------------------------------------------------------------- ref_sq_edges
def test_edges_only_index_files_within_the_size_caps():
    names = sorted(os.listdir(os.path.join(GOLD, "ref_sq_edges")))
    assert names == sorted(t + ".faiss" for t in sd.TAGS)
    sizes = [os.path.getsize(os.path.join(GOLD, "ref_sq_edges", n)) for n in names]
    sizes.append(os.path.getsize(os.path.join(GOLD, "ref_sq_edges.npz")))
    assert max(sizes) < 800_000 and sum(sizes) < 2_000_000


@pytest.mark.parametrize("tag", sd.TAGS)
def test_edges_files_are_the_named_cases(amd, ex, tag):
    qtype, l2, br, d, lens, _ = sd.CASES[tag]
    idx = amd.read_index(os.path.join(GOLD, "ref_sq_edges", tag + ".faiss"))
    assert type(idx) is amd.IndexIVFScalarQuantizer
    assert (idx.qtype, idx.by_residual, idx.d, idx.metric_type) == (qtype, bool(br), d, l2)
    assert [idx.get_list_size(l) for l in range(idx.nlist)] == lens
    assert list(ex[f"{tag}_meta"][:6]) == [d, len(lens), sum(lens), qtype, l2, br]
    tr = idx.sq_trained()
    if qtype == sd.QT_8bit:
        assert tr[d + 1] == 0 and (np.delete(tr[d:], 1) > 0).all()  # one constant dimension
        codes = np.concatenate([idx.list_codes(l) for l in range(idx.nlist)])
        assert (codes[1::2] == 0).any() and (codes[1::2] == 255).any()  # clamped rows
        assert (codes[:, 1] == 0).all()
    if "special" in tag:
        h = np.concatenate([idx.list_codes(l) for l in range(idx.nlist)]).view("<f2")
        assert np.isposinf(h).sum() >= 4 and np.isneginf(h).sum() >= 2 and np.isnan(h).any()
        sub = (h != 0) & (np.abs(h.astype(np.float32)) < 6.2e-5)
        assert sub.any()  # a subnormal half; -0.0 where the row itself is stored
        assert br or (h.view(np.uint16) == 0x8000).any()


@pytest.mark.parametrize("tag", sd.TAGS)
def test_edges_search_preassigned(models, ex, tag):
    m = models("ref_sq_edges", tag)
    nb = int(ex[f"{tag}_meta"][2])
    xq, keys, cdis = ex[f"{tag}_xq"], ex[f"{tag}_keys"], ex[f"{tag}_cdis"]
    assert (keys[1] == keys[0][::-1]).all() and keys[2, 1] == -1 and keys[3, 0] == keys[3, -1]
    for k in (1, 10, 600, 2 * nb):
        D, I = m.search_preassigned(xq, k, keys, cdis)
        same(D, I, ex[f"{tag}_pre_{k}_D"], ex[f"{tag}_pre_{k}_I"], k)
    # k = 2 nb: every admitted row, then the padding
    Ir = ex[f"{tag}_pre_{2 * nb}_I"]
    assert (Ir[:, -1] == -1).all()
    if "special" not in tag:
        longest = m.ids[-1].size
        assert ((Ir >= 0).sum(axis=1) == [nb, nb, nb - m.ids[1].size, nb + longest, nb, nb]).all()


def test_edges_ties_at_the_kth_place(ex):
    """in every case some query's group of equal distances is cut by k"""
    for tag in sd.TAGS:
        Dall = ex[f"{tag}_pre_{2 * int(ex[f'{tag}_meta'][2])}_D"]
        cut = 0
        for k in (1, 10, 600):
            Dk = ex[f"{tag}_pre_{k}_D"]
            cut += sum((Dall[q] == Dk[q, k - 1]).sum() > (Dk[q] == Dk[q, k - 1]).sum()
                       for q in range(sd.NQ))
        assert cut >= 1, tag


def test_edges_nonfinite_answers(ex):
    """what the reference returns on non-finite distances"""
    nb = 1282
    D = ex[f"sqfp16_l2_special_d8_pre_{2 * nb}_D"]
    I = ex[f"sqfp16_l2_special_d8_pre_{2 * nb}_I"]
    scanned = np.array([nb, nb, nb - 1, nb + 513, nb, nb])  # (a -1 probe; a list twice)
    assert np.isfinite(D[I >= 0]).all() and ((I >= 0).sum(axis=1) < scanned).all()  # L2: never
    D = ex[f"sqfp16_ip_special_d8_pre_{2 * nb}_D"]
    I = ex[f"sqfp16_ip_special_d8_pre_{2 * nb}_I"]
    assert np.isposinf(D[I >= 0]).any()          # inner product: +inf is returned ...
    assert not np.isneginf(D[I >= 0]).any() and not np.isnan(D[I >= 0]).any()  # ... these never
    D1 = ex["sqfp16_ip_special_d8_pre_1_D"]
    tied = [q for q in range(sd.NQ) if np.isposinf(D1[q, 0]) and np.isposinf(D[q]).sum() > 1]
    assert tied  # k = 1 cuts a group of +inf rows


@pytest.mark.parametrize("tag", sd.PARAM_TAGS)
def test_edges_store_pairs_max_codes_selector(models, ex, tag):
    m = models("ref_sq_edges", tag)
    xq = ex[f"{tag}_xq"]
    D, I = m.search_preassigned(xq, 10, ex[f"{tag}_keys"], ex[f"{tag}_cdis"], store_pairs=True)
    same(D, I, ex[f"{tag}_sp_10_D"], ex[f"{tag}_sp_10_I"], "sp")
    # IndexIVF::search on the reference's own probes (nprobe = nlist)
    Iq, Dq = ex[f"{tag}_q_I"], ex[f"{tag}_q_D"]
    sel = set(np.sort(ex[f"{tag}_ids"].astype(np.int64))[::2].tolist())
    for mc in sd.MAX_CODES:
        D, I = m.search_preassigned(xq, 10, Iq, Dq, max_codes=mc)
        same(D, I, ex[f"{tag}_params_mc{mc}_D"], ex[f"{tag}_params_mc{mc}_I"], mc)
    D, I = m.search_preassigned(xq, 10, Iq, Dq, sel=sel)
    same(D, I, ex[f"{tag}_params_sel_D"], ex[f"{tag}_params_sel_I"], "sel")
    D, I = m.search_preassigned(xq, 10, Iq, Dq, sel=sel, max_codes=300)
    same(D, I, ex[f"{tag}_params_mc300_sel_D"], ex[f"{tag}_params_mc300_sel_I"], "mc300 sel")


# ---------------------------------------------------------------- host side
@pytest.mark.parametrize("tag", sd.TAGS)
def test_edges_write_back_same_bytes(amd, tag, tmp_path):
    src = os.path.join(GOLD, "ref_sq_edges", tag + ".faiss")
    idx = amd.read_index(src)
    out = tmp_path / "out.faiss"
    amd.write_index(idx, out)
    assert out.read_bytes() == open(src, "rb").read()  # the by-residual byte included


@pytest.mark.parametrize("tag", sd.TAGS)
def test_edges_host_encode_gives_the_committed_codes(amd, orc, models, ex, tag, tmp_path):
    """add_core into the hand-laid empty index: this library's host encode, and
    the model's, against the codes the reference wrote"""
    c = sd.make(orc.float_rand, tag)
    assert np.array_equal(sd.sha(c["xb"]), ex[f"{tag}_xb_sha"]), "not the recorded input"
    empty = tmp_path / "empty.faiss"
    empty.write_bytes(sd.empty_iwsq(c["d"], c["qtype"], c["l2"], c["by_residual"], c["cent"],
                                    c["trained"]))
    idx = amd.read_index(empty)
    assert idx.by_residual == bool(c["by_residual"]) and idx.ntotal == 0
    idx.add_core(c["xb"], ex[f"{tag}_ids"].astype(np.int64), c["lists"])
    out = tmp_path / "filled.faiss"
    amd.write_index(idx, out)
    assert out.read_bytes() == open(os.path.join(GOLD, "ref_sq_edges", tag + ".faiss"), "rb").read()
    m = models("ref_sq_edges", tag)
    np.testing.assert_array_equal(m.encode(c["xb"], c["lists"]), np.concatenate(m.codes))
    np.testing.assert_array_equal(ex[f"{tag}_ids"], np.concatenate(m.ids))
