"""The linear-transform kernel (csrc/kernels_transform.hip) and IndexPreTransform
on the GPU.

Kernel against float64 with the standard fp32 dot-product bound, per output:
|y - y64| <= (K + 2) 2^-24 (|b| + sum_j |A_oj| |x_ij|), K the reduction length
(the transposed form's input fl(y - b) adds one rounding: K + 3).  A row's
result must have the same bits in any batch and on either tile shape, and an
IndexPreTransform must answer exactly as its sub-index does on apply_chain.

Files the reference trained and wrote (scripts/make_golden_pretransform.py):
its sgemm applies the transform in another order, so a query's ids are
compared only where every gap of the reference's top 11 exceeds what the two
roundings can move a distance (pretransform_bound.py); at most 10 % of the
queries may be set aside, and compared distances agree within that bound."""
import functools
import os

import numpy as np
import pytest
import torch

import hard_data as hd
from conftest import device_search, rand
from pretransform_bound import comparable, distance_move

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
GRID = [(4, 4), (6, 3), (36, 33), (64, 32), (130, 96), (264, 264)]
NROWS = 257


def ld4(d):
    return (d + 3) // 4 * 4


@functools.lru_cache(maxsize=None)
def case(d_in, d_out, transposed):
    """Signed, offset rows, a signed matrix and bias; the float64 result and
    the magnitude sum of the bound, computed once for the 257 rows."""
    A = hd.make("signed", d_out, d_in, 12)
    b = hd.make("signed", 1, d_out, 13)[0] + np.float32(0.5)
    k_len = d_out if transposed else d_in
    x = hd.make("signed", NROWS, k_len, 11) + np.float32(4.0)
    A64, x64 = A.astype(np.float64), x.astype(np.float64)
    return x, A, b, A64, x64


def reference(d_in, d_out, transposed, bias):
    x, A, b, A64, x64 = case(d_in, d_out, transposed)
    b64 = b.astype(np.float64) if bias else np.zeros(d_out)
    if transposed:
        y64 = (x64 - b64) @ A64
        mag = np.abs(x64 - b64) @ np.abs(A64)
        return y64, (d_out + 3) * EPS * mag
    y64 = x64 @ A64.T + b64
    return y64, (d_in + 2) * EPS * (np.abs(b64) + np.abs(x64) @ np.abs(A64).T)


def run(amd, rows, d_in, d_out, transposed, bias, variant=0):
    """The kernel on `rows`; input pad columns hold NaN (they must not be
    read), the output starts as NaN (every column must be written)."""
    _, A, b, _, _ = case(d_in, d_out, transposed)
    k_len, n_out = (d_out, d_in) if transposed else (d_in, d_out)
    n = rows.shape[0]
    xin = torch.full((n, ld4(k_len)), float("nan"), device="cuda")
    xin[:, :k_len] = torch.from_numpy(rows).cuda()
    out = torch.full((n, ld4(n_out)), float("nan"), device="cuda")
    dA, db = torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda()
    amd.linear_transform_device(xin.data_ptr(), n, ld4(k_len), dA.data_ptr(), d_in, d_out,
                                db.data_ptr() if bias else 0, out.data_ptr(), ld4(n_out),
                                transposed=transposed, variant=variant,
                                stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n", [1, 31, 33, 257])
@pytest.mark.parametrize("d_in,d_out", GRID)
def test_kernel_against_float64(amd, gpu, d_in, d_out, n, transposed, bias):
    x = case(d_in, d_out, transposed)[0]
    y64, bound = reference(d_in, d_out, transposed, bias)
    n_out = d_in if transposed else d_out
    y = run(amd, x[:n], d_in, d_out, transposed, bias)
    err = np.abs(y[:, :n_out].astype(np.float64) - y64[:n])
    print(f"max err / bound = {(err / bound[:n]).max():.3f}")
    assert (err <= bound[:n]).all()
    assert (y[:, n_out:].view(np.uint32) == 0).all()


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("d_in,d_out", GRID)
def test_batch_independence_bit_for_bit(amd, gpu, d_in, d_out, transposed):
    x = case(d_in, d_out, transposed)[0]
    full = run(amd, x, d_in, d_out, transposed, True).view(np.uint32)
    for r in (0, 31, 32, 256):
        alone = run(amd, x[r:r + 1], d_in, d_out, transposed, True).view(np.uint32)
        assert np.array_equal(alone[0], full[r]), r
    tail = run(amd, x[200:], d_in, d_out, transposed, True).view(np.uint32)
    assert np.array_equal(tail, full[200:])
    # the two tile shapes, each forced on the batch size the other serves
    assert np.array_equal(run(amd, x, d_in, d_out, transposed, True, 2).view(np.uint32), full)
    assert np.array_equal(run(amd, x[:1], d_in, d_out, transposed, True, 1).view(np.uint32),
                          full[:1])


D_IN, D_SUB, NB, NQ, K = 40, 32, 2000, 50, 10


@functools.lru_cache(maxsize=None)
def composition_data():
    rng = np.random.default_rng(5)
    q, _ = np.linalg.qr(rng.standard_normal((D_IN, D_IN)))
    A = np.ascontiguousarray(q[:D_SUB], dtype=np.float32)  # orthonormal rows
    b = rng.standard_normal(D_SUB).astype(np.float32)
    xb = hd.make("signed", NB, D_IN, 21) + np.float32(1.0)
    xq = hd.queries("signed", xb, NQ, 22)
    return A, b, xb, xq


@pytest.fixture(scope="module", params=["IVF16,Flat", "IVF16,PQ8", "Flat"])
def composed(request, amd, gpu):
    A, b, xb, xq = composition_data()
    lt = amd.LinearTransform(A=A, b=b)
    base = amd.index_factory(D_SUB, request.param)
    idx = amd.IndexPreTransform(lt, base)
    idx.train(xb)
    idx.add(xb)
    if request.param != "Flat":
        base.nprobe = 4
        base.make_direct_map()
    assert idx.ntotal == base.ntotal == NB and idx.d == D_IN and lt.is_orthonormal
    return idx, base, lt


def test_search_equals_base_on_apply_chain(composed):
    idx, base, _ = composed
    xq = composition_data()[3]
    xt = idx.apply_chain(xq)
    D, I = idx.search(xq, K)
    Db, Ib = base.search(xt, K)
    assert np.array_equal(I, Ib) and np.array_equal(D.view(np.uint32), Db.view(np.uint32))
    Dd, Id = device_search(idx, xq, K)
    assert np.array_equal(Id, Ib) and np.array_equal(Dd.view(np.uint32), Db.view(np.uint32))
    radius = float(np.median(D[:, K // 2]))
    for got, want in zip(idx.range_search(xq, radius), base.range_search(xt, radius)):
        assert np.array_equal(got, want)
    assert idx.range_search(xq, radius)[0][-1] > 0


def test_chain_of_two_equals_by_hand(composed, amd):
    idx, base, lt = composed
    rng = np.random.default_rng(6)
    lt2 = amd.LinearTransform(A=rng.standard_normal((D_IN, 46)).astype(np.float32))
    two = amd.IndexPreTransform(lt, base)
    two.prepend_transform(lt2)
    x = hd.make("signed", 70, 46, 23)
    assert two.d == 46 and [t.d_in for t in two.chain] == [46, D_IN]
    assert np.array_equal(two.apply_chain(x).view(np.uint32),
                          lt.apply(lt2.apply(x)).view(np.uint32))
    D, I = two.search(x, K)
    Db, Ib = base.search(two.apply_chain(x), K)
    assert np.array_equal(I, Ib) and np.array_equal(D.view(np.uint32), Db.view(np.uint32))


def test_reconstruct_through_reverse_chain(composed):
    idx, base, _ = composed
    A, b = composition_data()[:2]
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    for i in (0, 7, NB - 1):
        r = base.reconstruct(i)
        got = idx.reconstruct(i)
        assert np.array_equal(got.view(np.uint32), idx.reverse_chain(r[None])[0].view(np.uint32))
        u = r.astype(np.float64) - b64
        bound = (D_SUB + 3) * EPS * (np.abs(u) @ np.abs(A64))
        assert (np.abs(got - u @ A64) <= bound).all()
    assert np.array_equal(idx.reconstruct_n(3, 5).view(np.uint32),
                          idx.reverse_chain(base.reconstruct_n(3, 5)).view(np.uint32))


@pytest.mark.parametrize("tag", ["opq8_32_ivf16_pq8", "pca24_ivf16_flat"])
def test_reference_written_file(amd, orc, gpu, tag):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pretransform")
    fx = np.load(os.path.join(here, tag + ".npz"))
    seed, nb, nq, k11 = (int(v) for v in fx["meta"])
    idx = amd.read_index(os.path.join(here, tag + ".faiss"))
    assert idx.ntotal == nb and idx.is_trained
    xq = rand(orc, nq, idx.d, seed + 1000)
    t, = idx.chain
    A = t.A.reshape(t.d_out, t.d_in)
    b = t.b if t.have_bias else np.zeros(t.d_out, np.float32)
    keep = comparable(xq, A, b, fx["D"])
    assert (~keep).sum() <= nq // 10
    D, I = idx.search(xq, k11 - 1)
    Dr, Ir = fx["D"][:, :-1], fx["I"][:, :-1]
    assert np.array_equal(I[keep], Ir[keep])
    move = distance_move(xq, A, b, Dr)
    assert (np.abs(D.astype(np.float64) - Dr)[keep] <= move[keep]).all()
