"""IndexFlat's other metrics on the CPU side: IxFl files built by hand from the
reference's layout (faiss/impl/index_write.cpp:79-90, 396-403), and the refusals."""
import struct

import numpy as np
import pytest


def flat_bytes(tag, xb, metric, arg=0.0):
    n, d = xb.shape
    hdr = struct.pack("<iqqqBi", d, n, 1 << 20, 1 << 20, 1, metric)
    if metric > 1:
        hdr += struct.pack("<f", arg)
    return tag + hdr + struct.pack("<Q", n * d) + xb.astype("<f4").tobytes()


XB = (np.arange(40, dtype=np.float32).reshape(5, 8) - 11) / 4


@pytest.mark.parametrize("tag,metric,arg,out_tag", [
    (b"IxFl", 2, 0.0, b"IxFl"), (b"IxFl", 4, 3.0, b"IxFl"), (b"IxF2", 2, 0.0, b"IxFl"),
    (b"IxF2", 1, 0.0, b"IxF2"), (b"IxFI", 0, 0.0, b"IxFI")])
def test_flat_file_round_trip(amd, tmp_path, tag, metric, arg, out_tag):
    src, dst = tmp_path / "in.index", tmp_path / "out.index"
    src.write_bytes(flat_bytes(tag, XB, metric, arg))
    idx = amd.read_index(src)
    assert type(idx).__name__ == "IndexFlat" and (idx.d, idx.ntotal) == (8, 5)
    assert idx.metric_type == metric and idx.metric_arg == arg
    assert np.array_equal(idx.reconstruct(3), XB[3])
    amd.write_index(idx, dst)
    assert dst.read_bytes() == flat_bytes(out_tag, XB, metric, arg)


def test_metric_arg_and_factory(amd):
    idx = amd.index_factory(8, "Flat", amd.METRIC_Jaccard)
    idx.metric_arg = 2.5
    assert type(idx).__name__ == "IndexFlat" and (idx.metric_type, idx.metric_arg) == (23, 2.5)


@pytest.mark.parametrize("make", [
    lambda amd: amd.IndexIVFFlat(amd.IndexFlat(8), 8, 4, 2),
    lambda amd: amd.IndexHNSWFlat(8, 16, 2),
    lambda amd: amd.IndexPQ(8, 2, 8, 2),
    lambda amd: amd.index_factory(8, "IVF4,Flat", 2),
    lambda amd: amd.IndexRefineFlat(amd.IndexFlat(8, 2))])
def test_other_classes_refuse_the_metric(amd, make):
    with pytest.raises(amd.FaissError, match="METRIC_L2 and METRIC_INNER_PRODUCT only"):
        make(amd)
