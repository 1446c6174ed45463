"""Editing an index on the host: remove_ids, the direct maps, reconstruct /
reconstruct_n / reconstruct_from_offset and their file format, against what
the reference CPU library left for the same operations on the same files
(tests/golden/ref_mutation*, scripts/make_golden_mutation.py).  Everything is
compared bit for bit.  No GPU needed: the indexes are read from the
reference's own files.  (update_vectors assigns the new vectors with the
coarse quantizer, which runs on the GPU: tests/test_gpu_ivf_mutation.py.)"""
import ctypes as C

import numpy as np
import pytest

from mutation_data import REMOVALS, TAGS, assert_lists, fixtures, map_pairs, path, selector, text


@pytest.fixture(scope="module")
def fx():
    return fixtures()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- removal
@pytest.mark.parametrize("tag", TAGS)
def test_base_lists(amd, fx, tag):
    idx = amd.read_index(path(tag))
    assert idx.direct_map_type == amd.DIRECT_MAP_NONE
    assert_lists(idx, fx, f"{tag}_base")


@pytest.mark.parametrize("how", REMOVALS)
@pytest.mark.parametrize("tag", TAGS)
def test_remove_without_map(amd, fx, tag, how):
    idx = amd.read_index(path(tag))
    n0 = idx.ntotal
    nrm = idx.remove_ids(selector(amd, fx, tag, how))
    count, ntotal = (int(v) for v in fx[f"{tag}_rm_{how}_count"])
    assert (nrm, idx.ntotal) == (count, ntotal) and n0 - nrm == ntotal
    assert_lists(idx, fx, f"{tag}_rm_{how}")


def test_remove_ids_takes_an_id_array(amd, fx):
    idx = amd.read_index(path("pq8"))
    assert idx.remove_ids(fx["pq8_rm_array_sel"]) == int(fx["pq8_rm_array_count"][0])
    assert_lists(idx, fx, "pq8_rm_array")


@pytest.mark.parametrize("tag", TAGS)
def test_remove_through_hashtable(amd, fx, tag):
    idx = amd.read_index(path(tag))
    idx.set_direct_map_type(amd.DIRECT_MAP_HASHTABLE)
    assert idx.direct_map_type == amd.DIRECT_MAP_HASHTABLE
    nrm = idx.remove_ids(selector(amd, fx, tag, "hash"))  # repeats an id, names an absent one
    count, ntotal = (int(v) for v in fx[f"{tag}_rm_hash_count"])
    assert (nrm, idx.ntotal) == (count, ntotal)
    assert_lists(idx, fx, f"{tag}_rm_hash")
    want = fx[f"{tag}_hash_map"]
    assert len(want) == ntotal
    assert np.array_equal(map_pairs(idx, range(0, 2000 + 3001)), want)
    with pytest.raises(amd.FaissError) as e:
        idx.remove_ids(amd.IDSelectorRange(0, 10))
    assert text(fx[f"{tag}_hash_refusal"]).split("failed: ")[-1] in str(e.value)
    assert "remove with hashtable works only with IDSelectorArray" in str(e.value)
    assert idx.ntotal == ntotal


@pytest.mark.parametrize("tag", TAGS)
def test_array_map_refuses_removal(amd, fx, tag):
    idx = amd.read_index(path(tag))
    idx.make_direct_map(True)
    assert idx.direct_map_type == amd.DIRECT_MAP_ARRAY
    with pytest.raises(amd.FaissError) as e:
        idx.remove_ids(amd.IDSelectorRange(0, 10))
    msg = "remove not supported with this direct_map format"
    assert msg in text(fx[f"{tag}_array_refusal"]) and msg in str(e.value)
    assert idx.ntotal == 2000
    assert_lists(idx, fx, f"{tag}_base")


# ---------------------------------------------------------------- the map
def test_map_contents_and_messages(amd, fx):
    idx = amd.read_index(path("flat"))
    with pytest.raises(amd.FaissError, match="direct map not initialized"):
        idx.direct_map_get(3)
    idx.make_direct_map(True)
    for l in range(idx.nlist):
        for o, i in enumerate(idx.list_ids(l)):
            assert idx.direct_map_get(i) == (l, o)
    for bad in (-1, 2000):
        with pytest.raises(amd.FaissError, match="invalid key"):
            idx.direct_map_get(bad)
    idx.make_direct_map(False)
    assert idx.direct_map_type == amd.DIRECT_MAP_NONE
    idx.set_direct_map_type(amd.DIRECT_MAP_HASHTABLE)
    assert idx.direct_map_get(1999) == idx.direct_map_get(1999)
    with pytest.raises(amd.FaissError, match="key not found"):
        idx.direct_map_get(2000)
    # reset() clears the contents and keeps the type
    idx.reset()
    assert idx.direct_map_type == amd.DIRECT_MAP_HASHTABLE and idx.ntotal == 0
    with pytest.raises(amd.FaissError, match="key not found"):
        idx.direct_map_get(0)


def test_array_map_needs_sequential_ids(amd, fx):
    idx = amd.read_index(path("pq8"))
    idx.remove_ids(amd.IDSelectorRange(0, 10))  # ids up to 1999 stay, ntotal is 1990
    with pytest.raises(amd.FaissError, match="direct map supported only for seuquential ids"):
        idx.make_direct_map(True)


def test_array_map_with_removed_entry_reports_minus_one(amd, fx):
    """An Array entry of -1 (a vector the quantizer assigned to no list) is
    the reference's '-1 entry in direct_map'."""
    import struct
    raw = bytearray(open(path("pq8_array"), "rb").read())
    idx = amd.read_index(path("pq8_array"))
    KEY = 11
    arr = np.array([(l << 32) | o for l, o in map(idx.direct_map_get, range(2000))], np.int64)
    at = bytes(raw).find(arr.tobytes())  # the map's array in the file
    assert at > 0
    at += 8 * KEY
    raw[at:at + 8] = struct.pack("<q", -1)
    import tempfile
    with tempfile.NamedTemporaryFile(suffix=".faiss") as f:
        f.write(raw)
        f.flush()
        idx2 = amd.read_index(f.name)
    with pytest.raises(amd.FaissError, match="-1 entry in direct_map"):
        idx2.direct_map_get(KEY)
    with pytest.raises(amd.FaissError, match="-1 entry in direct_map"):
        idx2.reconstruct(KEY)


# ---------------------------------------------------------------- reconstruct
@pytest.mark.parametrize("tag", TAGS)
def test_reconstruct_through_map(amd, fx, tag):
    idx = amd.read_index(path(tag))
    keys, want = fx[f"{tag}_rec_keys"], fx[f"{tag}_rec_x"]
    if tag == "flat":  # the map-less walk over the lists stays
        assert np.array_equal(bits(idx.reconstruct(int(keys[0]))), want[0])
    else:
        with pytest.raises(amd.FaissError, match="direct map not initialized"):
            idx.reconstruct(int(keys[0]))
    for kind in (amd.DIRECT_MAP_ARRAY, amd.DIRECT_MAP_HASHTABLE):
        idx.set_direct_map_type(kind)
        for key, w in zip(keys, want):
            assert np.array_equal(bits(idx.reconstruct(int(key))), w), (tag, kind, key)
            l, o = idx.direct_map_get(int(key))
            assert np.array_equal(bits(idx.reconstruct_from_offset(l, o)), w)


@pytest.mark.parametrize("tag", TAGS)
def test_reconstruct_n_after_removal(amd, fx, tag):
    idx = amd.read_index(path(tag))
    idx.remove_ids(selector(amd, fx, tag, "range"))
    i0, ni = (int(v) for v in fx[f"{tag}_recn_range"])
    want = fx[f"{tag}_recn_x"]
    out = np.full((ni, idx.d), 0x7fc0dead, np.uint32).view(np.float32)
    idx.reconstruct_n(i0, ni, out)
    assert np.array_equal(out.view(np.uint32), want)
    assert (want == 0x7fc0dead).all(axis=1).sum() == 100  # the removed ids' rows: untouched
    with pytest.raises(amd.FaissError):
        idx.reconstruct_n(idx.ntotal - 5, 6)


def test_reconstruct_from_offset_every_row(amd, fx):
    """pq12x5: 60-bit codes, fields straddle bytes; every row through the map
    equals the row by offset, and rows of duplicate vectors' codes decode alike."""
    idx = amd.read_index(path("pq12x5"))
    idx.make_direct_map(True)
    for l in range(idx.nlist):
        ids = idx.list_ids(l)
        for o in range(0, len(ids), 7):
            assert np.array_equal(bits(idx.reconstruct_from_offset(l, o)),
                                  bits(idx.reconstruct(int(ids[o]))))
    with pytest.raises(amd.FaissError):
        idx.reconstruct_from_offset(0, idx.get_list_size(0))
    with pytest.raises(amd.FaissError):
        idx.reconstruct_from_offset(idx.nlist, 0)


def test_sq8_decode_is_the_reference_formula(amd, fx):
    """ScalarQuantizer::decode for all 256 codes x 8 (vmin, vdiff) pairs:
    xi = (code + 0.5f) / 255.0f, x = fma(xi, vdiff, vmin).  The fixture's
    generator found this the only candidate that reproduces the table; here
    the library's reconstruct is run on an index whose trained ranges are the
    table's (an IwSq file patched from sq8.faiss)."""
    assert str(fx["sq_formula"]) == "div_fma"
    vmin, vdiff, want = fx["sq_vmin"], fx["sq_vdiff"], fx["sq_decode"]
    idx = amd.read_index(path("sq8"))
    d = idx.d
    tr = idx.sq_trained().copy()
    raw = bytearray(open(path("sq8"), "rb").read())
    at = bytes(raw).find(tr.tobytes())
    assert at > 0
    reps = d // 8
    new = np.concatenate([np.tile(vmin, reps), np.tile(vdiff, reps)]).astype(np.float32)
    raw[at:at + new.nbytes] = new.tobytes()
    # by_residual off: the byte after the trained vector and code_size
    by_res_at = at + new.nbytes + 8
    assert raw[by_res_at] == 1
    raw[by_res_at] = 0
    # the first list's first 256 rows' codes -> code c in every component
    l = int(np.argmax([idx.get_list_size(i) for i in range(idx.nlist)]))
    n = idx.get_list_size(l)
    codes = idx.list_codes(l)
    cat = bytes(raw).find(codes.tobytes())
    assert cat > 0
    m = min(n, 256)
    first = np.repeat(np.arange(m, dtype=np.uint8)[:, None], d, axis=1)
    second = np.repeat(np.arange(256 - m, 256, dtype=np.uint8)[:, None], d, axis=1)
    seen = np.zeros(256, bool)
    import tempfile
    for block in (first, second):
        raw[cat:cat + block.size] = block.tobytes()
        with tempfile.NamedTemporaryFile(suffix=".faiss") as f:
            f.write(raw)
            f.flush()
            idx2 = amd.read_index(f.name)
        for o in range(len(block)):
            c = int(block[o, 0])
            got = bits(idx2.reconstruct_from_offset(l, o))
            assert np.array_equal(got, np.tile(want[c], reps)), c
            seen[c] = True
    assert seen.all()


# ---------------------------------------------------------------- files
def test_array_map_file_round_trip(amd, fx, tmp_path):
    src = path("pq8_array")
    idx = amd.read_index(src)
    assert idx.direct_map_type == amd.DIRECT_MAP_ARRAY
    out = tmp_path / "a.faiss"
    amd.write_index(idx, str(out))
    assert out.read_bytes() == open(src, "rb").read()
    # no map: byte-identical too
    idx = amd.read_index(path("pq8"))
    amd.write_index(idx, str(out))
    assert out.read_bytes() == open(path("pq8"), "rb").read()
    # a map made here gives the reference's file (whose nprobe the driver set to 4)
    idx.make_direct_map(True)
    idx.nprobe = 4
    amd.write_index(idx, str(out))
    assert out.read_bytes() == open(src, "rb").read()


@pytest.mark.parametrize("tag", ["flat", "sq8"])
def test_array_map_file_other_classes(amd, tag, tmp_path):
    idx = amd.read_index(path(tag))
    idx.make_direct_map(True)
    out = tmp_path / "a.faiss"
    amd.write_index(idx, str(out))
    idx2 = amd.read_index(str(out))
    assert idx2.direct_map_type == amd.DIRECT_MAP_ARRAY
    assert all(idx2.direct_map_get(i) == idx.direct_map_get(i) for i in range(0, 2000, 13))
    out2 = tmp_path / "b.faiss"
    amd.write_index(idx2, str(out2))
    assert out2.read_bytes() == out.read_bytes()


def test_hashtable_file_round_trip_by_content(amd, fx, tmp_path):
    src = path("pq8_hash")
    idx = amd.read_index(src)
    assert idx.direct_map_type == amd.DIRECT_MAP_HASHTABLE
    ref = amd.read_index(path("pq8"))
    ref.set_direct_map_type(amd.DIRECT_MAP_HASHTABLE)
    ids = range(0, 2005)
    want = map_pairs(ref, ids)
    assert len(want) == 2000 and np.array_equal(map_pairs(idx, ids), want)
    out = tmp_path / "h.faiss"
    amd.write_index(idx, str(out))
    raw, sraw = out.read_bytes(), open(src, "rb").read()
    assert len(raw) == len(sraw)
    # the pairs are written in ascending id order
    at = raw.find(want[:3].tobytes())
    assert at > 0 and raw[at:at + want.nbytes] == want.tobytes()
    assert raw[:at] == sraw[:at] and raw[at + want.nbytes:] == sraw[at + want.nbytes:]
    idx2 = amd.read_index(str(out))
    assert np.array_equal(map_pairs(idx2, ids), want)
    assert_lists(idx2, fx, "pq8_base")
    # clone_index goes through the file and keeps the map
    cl = amd.clone_index(idx)
    assert cl.direct_map_type == amd.DIRECT_MAP_HASHTABLE
    assert np.array_equal(map_pairs(cl, ids), want)


def test_copy_subset_and_shards_refuse_a_map(amd, fx):
    src = amd.read_index(path("flat"))
    dst = amd.read_index(path("flat"))
    dst.reset()
    dst.make_direct_map(True)
    with pytest.raises(amd.FaissError, match="direct map"):
        amd.copy_subset_to(src, dst, 0, 0, 100)
    assert dst.ntotal == 0
    src.set_direct_map_type(amd.DIRECT_MAP_HASHTABLE)
    with pytest.raises(amd.FaissError, match="direct map"):
        amd.index_ivf_to_shards(src, 2, 1)


# ---------------------------------------------------------------- other classes
def test_index_flat_remove_ids(amd):
    rng = np.random.default_rng(5)
    xb = rng.standard_normal((50, 12), dtype=np.float32)
    f = amd.IndexFlatL2(12)
    f.add(xb)
    # the selector is asked about row numbers; survivors keep their order
    assert f.remove_ids(amd.IDSelectorBatch([3, 4, 49, 77])) == 3
    keep = np.array([i for i in range(50) if i not in (3, 4, 49)])
    assert f.ntotal == 47 and np.array_equal(f.xb, xb[keep])
    assert np.array_equal(f.reconstruct(3), xb[5])
    assert f.remove_ids(amd.IDSelectorRange(0, 47)) == 47 and f.ntotal == 0
    assert f.remove_ids([1, 2]) == 0
    assert np.array_equal(f.reconstruct_n(0, 0), np.zeros((0, 12), np.float32))


def test_types_without_removal_throw_the_base_message(amd, fx):
    import os
    gold = os.path.join(os.path.dirname(path("flat")), "..")
    msg = "remove_ids not implemented for this type of index"
    hn = amd.read_index(os.path.join(gold, "ref_full", "hnsw_dup.faiss"))
    rf = amd.read_index(os.path.join(gold, "ref_refine", "pq_l2_d64.faiss"))
    sh = amd.index_ivf_to_shards(amd.read_index(path("flat")), 2, 1)
    for ix in (hn, rf, sh):
        n0 = ix.ntotal
        with pytest.raises(amd.FaissError, match=msg):
            ix.remove_ids(amd.IDSelectorRange(0, 5))
        assert ix.ntotal == n0


def test_mapped_lists_refuse_mutation(amd, fx):
    idx = amd.read_index(path("flat"), amd.IO_FLAG_MMAP)
    with pytest.raises(amd.FaissError, match="mapped from .*flat.faiss"):
        idx.remove_ids(amd.IDSelectorRange(0, 10))
    idx.make_direct_map(True)  # reading the lists is fine
    with pytest.raises(amd.FaissError, match="mapped from"):
        idx.update_vectors([1], np.zeros((1, idx.d), np.float32))
    assert idx.ntotal == 2000
    assert_lists(idx, fx, "flat_base")
    idx.make_direct_map(False)
    idx.materialize_invlists()
    assert idx.remove_ids(selector(amd, fx, "flat", "range")) == int(fx["flat_rm_range_count"][0])
    assert_lists(idx, fx, "flat_rm_range")


# ---------------------------------------------------------------- C entry points
def test_c_entry_points(amd, fx):
    L = amd.lib()
    h = C.c_void_p()
    assert L.faiss_read_index_fname(path("sq8").encode(), 0, C.byref(h)) == 0
    try:
        ids = np.ascontiguousarray(fx["sq8_rm_array_sel"], dtype=np.int64)
        sel = C.c_void_p()
        assert L.faiss_IDSelectorArray_new(C.byref(sel), len(ids), ids.ctypes.data_as(C.c_void_p)) == 0
        n = C.c_size_t(0)
        assert L.faiss_IndexIVF_make_direct_map(h, 1) == 0
        assert L.faiss_amd_IndexIVF_direct_map_type(h) == 1
        assert L.faiss_Index_remove_ids(h, sel, C.byref(n)) == -2
        assert b"remove not supported with this direct_map format" in L.faiss_get_last_error()
        assert L.faiss_IndexIVF_make_direct_map(h, 0) == 0
        assert L.faiss_Index_remove_ids(h, sel, C.byref(n)) == 0
        assert n.value == int(fx["sq8_rm_array_count"][0])
        assert L.faiss_Index_ntotal(h) == int(fx["sq8_rm_array_count"][1])
        L.faiss_IDSelector_free(sel)
        assert L.faiss_amd_IndexIVF_set_direct_map_type(h, 2) == 0
        assert L.faiss_amd_IndexIVF_set_direct_map_type(h, 3) == -2
        lo = C.c_int64(0)
        assert L.faiss_amd_IndexIVF_direct_map_get(h, 0, C.byref(lo)) == 0
        d = L.faiss_Index_d(h)
        a = np.empty(d, np.float32)
        b = np.empty(d, np.float32)
        assert L.faiss_amd_IndexIVF_reconstruct_from_offset(
            h, lo.value >> 32, lo.value & 0xffffffff, a.ctypes.data_as(C.c_void_p)) == 0
        assert L.faiss_Index_reconstruct(h, 0, b.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # reconstruct_n is the index's own (one pass over the lists)
        out = np.zeros((3, d), np.float32)
        assert L.faiss_Index_reconstruct_n(h, 0, 3, out.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(out[0].view(np.uint32), b.view(np.uint32))
        assert L.faiss_Index_reconstruct_n(h, 0, 10 ** 6, out.ctypes.data_as(C.c_void_p)) == -2
        # update_vectors of a flat-only entry point refuses another class
        assert L.faiss_IndexIVFFlat_update_vectors(h, 0, None, None) == -2
        assert b"not an IndexIVFFlat" in L.faiss_get_last_error()
    finally:
        L.faiss_Index_free(h)
