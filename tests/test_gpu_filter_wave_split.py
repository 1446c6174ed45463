"""The streamed Flat filter's work-item mapping (kernels_ivf_mfma.hip
k_ivf_bf2_stream) against the oracle, bit for bit: how many of a group's four
waves an item's queries keep busy, and the last tile of a list, of which only
the blocks with real rows are copied and computed.  (Written for a split of
narrow items over (query slice, row block) wave pairs, which was measured
slower and dropped — DESIGN section 4; the cases are those of that change.)

Every list is probed (IVF16 with nprobe = 16), so each list's items see
exactly nq queries, split at 128: the widths cover every wave boundary (32,
64, 96, 128) and remainder items of 1, 32 and 65 queries.  Lists of about 200
rows give several tiles and a ragged last one; k = 1, 10, 20 are the 2, 4 and
8 key streams; d = 128, 64, 30 the 8, 4 and 2 k-step forms; inner product the
plain-key path; 12,000 rows the 8-keys-by-length path; an empty and a tiny
list, and lists of exactly 1 .. 256 rows, every form of the last tile;
IVF16,PQ16x8 with the image filter the PQ form of the same kernel.
"""
import numpy as np
import pytest

from conftest import assert_same_results, rand

pytestmark = pytest.mark.gpu

NLIST = 16
WIDTHS = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 193]
NQMAX = 193


def make(amd, desc, xb, train=None, metric=None):
    idx = (amd.index_factory(xb.shape[1], desc) if metric is None
           else amd.index_factory(xb.shape[1], desc, metric))
    idx.train(xb if train is None else train)
    idx.add(xb)
    idx.nprobe = NLIST
    return idx


class Case:
    """An index, its queries and the oracle's results for all of them (a
    query's result does not depend on the batch it is searched in)."""

    def __init__(self, amd, orc, idx, xq, ks):
        self.idx, self.xq = idx, xq
        ref = orc.IVFOracle.from_index(idx)
        self.ref = {k: ref.search(xq, k, NLIST, nslices=1)[:2] for k in ks}

    def check(self, nq, k):
        D, I = self.idx.search(np.ascontiguousarray(self.xq[:nq]), k)
        Dr, Ir = self.ref[k]
        assert_same_results(D, I, Dr[:nq], Ir[:nq])


def ran_stages(amd, idx, fn):
    amd.set_kernel_timing(True)
    try:
        idx.reset_kernel_times()
        out = fn()
        names = {nm for nm, _, _ in idx.kernel_times()}
    finally:
        amd.set_kernel_timing(False)
    return out, names


@pytest.fixture(scope="module")
def l2_128(amd, orc, gpu):
    xb, xq = rand(orc, 3200, 128, 5201), rand(orc, NQMAX, 128, 5202)
    return Case(amd, orc, make(amd, f"IVF{NLIST},Flat", xb), xq, (1, 10, 20))


@pytest.fixture(scope="module")
def ip_128(amd, orc, gpu):
    xb, xq = rand(orc, 3200, 128, 5203), rand(orc, NQMAX, 128, 5204)
    idx = make(amd, f"IVF{NLIST},Flat", xb, metric=amd.METRIC_INNER_PRODUCT)
    return Case(amd, orc, idx, xq, (10,))


@pytest.fixture(scope="module", params=[64, 30])
def l2_narrow_d(amd, orc, gpu, request):
    d = request.param
    xb, xq = rand(orc, 3200, d, 5205 + d), rand(orc, 129, d, 5206 + d)
    return Case(amd, orc, make(amd, f"IVF{NLIST},Flat", xb), xq, (10,))


@pytest.fixture(scope="module")
def long_lists(amd, orc, gpu):
    xb, xq = rand(orc, 12000, 128, 5209), rand(orc, 100, 128, 5210)
    # 750 rows per list on average (>= 512): 8 kept keys per stream at k = 10
    idx = make(amd, f"IVF{NLIST},Flat", xb)
    return Case(amd, orc, idx, xq, (10,))


@pytest.fixture(scope="module")
def ragged_lists(amd, orc, gpu):
    # trained on 14 base rows plus two far points: one far centroid attracts
    # only the 5 base rows moved next to it, the other nothing
    xb = rand(orc, 3200, 128, 5211).copy()
    far_a = np.full(128, 40.0, np.float32)
    far_b = np.full(128, -40.0, np.float32)
    xb[:5] = far_a + 0.01 * xb[:5]
    train = np.ascontiguousarray(np.vstack([xb[100:114], far_a[None], far_b[None]]))
    idx = make(amd, f"IVF{NLIST},Flat", xb, train=train)
    sizes = sorted(idx.get_list_size(l) for l in range(NLIST))
    assert sizes[0] == 0 and 0 < sizes[1] < 32, sizes
    return Case(amd, orc, idx, rand(orc, NQMAX, 128, 5212), (10,))


LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 191, 192, 193, 256]


@pytest.fixture(scope="module")
def exact_lengths(amd, orc, gpu):
    # 16 far-apart centroids (the training set itself), list l = LENGTHS[l]
    # rows next to centroid l: last tiles of 1, 31, 32, 33, 63 and 64 rows
    cent = np.ascontiguousarray(10.0 * rand(orc, NLIST, 128, 5215))
    noise = rand(orc, sum(LENGTHS), 128, 5216)
    xb = np.ascontiguousarray(np.repeat(cent, LENGTHS, axis=0) + 0.05 * noise)
    idx = make(amd, f"IVF{NLIST},Flat", xb, train=cent)
    assert sorted(idx.get_list_size(l) for l in range(NLIST)) == LENGTHS
    xq = np.ascontiguousarray(5.0 * rand(orc, 129, 128, 5217))
    return Case(amd, orc, idx, xq, (10,))


@pytest.fixture(scope="module")
def pq_image(amd, orc, gpu):
    # the switch is read when the index is uploaded (the first search) and at
    # every search: set for the fixture's lifetime
    mp = pytest.MonkeyPatch()
    mp.setenv("FAISS_AMD_PQ_FILTER", "image")
    try:
        xb, xq = rand(orc, 3200, 128, 5213), rand(orc, 129, 128, 5214)
        yield Case(amd, orc, make(amd, f"IVF{NLIST},PQ16x8", xb), xq, (10,))
    finally:
        mp.undo()


@pytest.mark.parametrize("k", [1, 10, 20])
@pytest.mark.parametrize("nq", WIDTHS)
def test_l2_widths(l2_128, nq, k):
    l2_128.check(nq, k)


def test_l2_runs_the_streamed_filter(amd, l2_128):
    c = l2_128
    _, names = ran_stages(amd, c.idx, lambda: c.idx.search(c.xq[:33].copy(), 10))
    assert "ivf_flat_scan" in names and "ivf_exact_scan" not in names, names
    # the last tile's forms: at most 32 real rows (its second block is
    # skipped) and more than 32 (both blocks, the padding rows masked)
    last = [(c.idx.get_list_size(l) - 1) % 64 + 1 for l in range(NLIST)]
    assert min(last) <= 32 < max(last), last


@pytest.mark.parametrize("nq", WIDTHS)
def test_inner_product_widths(ip_128, nq):
    ip_128.check(nq, 10)


@pytest.mark.parametrize("nq", [33, 64, 65, 129])
def test_narrow_dims(l2_narrow_d, nq):
    l2_narrow_d.check(nq, 10)


@pytest.mark.parametrize("nq", [40, 100])
def test_long_lists(long_lists, nq):
    long_lists.check(nq, 10)


@pytest.mark.parametrize("nq", WIDTHS)
def test_empty_and_tiny_lists(ragged_lists, nq):
    ragged_lists.check(nq, 10)


@pytest.mark.parametrize("nq", [33, 129])
def test_exact_list_lengths(exact_lengths, nq):
    exact_lengths.check(nq, 10)


@pytest.mark.parametrize("nq", [33, 65, 129])
def test_pq_image_form(amd, pq_image, nq):
    c = pq_image
    _, names = ran_stages(amd, c.idx, lambda: c.check(nq, 10))
    assert "ivfpq_filter" in names and "ivf_exact_scan" not in names, names
    assert c.idx.debug_rows(2)[0] == 2 * 128 + 16  # the decoded image exists
