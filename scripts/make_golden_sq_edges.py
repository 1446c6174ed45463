#!/usr/bin/env python3
"""Reference-run edge fixtures for IndexIVFScalarQuantizer.

Writes tests/golden/ref_sq_edges/<tag>.faiss (the reference's own write_index)
and tests/golden/ref_sq_edges.npz (the reference's search results).  Runs only
where oracle/_ref/libfaissfull.so exists, through the reff_* entry points it
already exports, with one OpenMP thread.

For each case of tests/sq_edges_data.py: the empty IwSq index is laid out by
hand (centroids, trained ranges, by-residual byte), the reference reads it,
encodes the rows into the chosen lists with add_core and writes the index; then
search_preassigned runs over six probe rows (in order, reversed, with a -1,
with the longest list named twice) and random coarse distances at
k = 1, 10, 600 and 2 nb.  Two cases add store_pairs, max_codes and an id-batch
selector of every second id through IndexIVF::search on the reference's own
coarse quantizer, whose probes are recorded too.

    python scripts/make_golden_sq_edges.py
"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import sq_edges_data as sd  # noqa: E402

OUTD = os.path.join(ROOT, "tests", "golden", "ref_sq_edges")
OUT = os.path.join(ROOT, "tests", "golden", "ref_sq_edges.npz")

L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libfaissfull.so"), mode=C.RTLD_GLOBAL)
P, I64 = C.c_void_p, C.c_int64
L.reff_last_error.restype = C.c_char_p
L.reff_read_index.restype = P
L.reff_read_index.argtypes = [C.c_char_p, C.c_int]
L.reff_write_index.argtypes = [P, C.c_char_p]
L.reff_free.argtypes = [P]
L.reff_add_core.argtypes = [P, I64, P, P, P]
L.reff_search_params.argtypes = [P, I64, P, I64, I64, I64, P, I64, P, P]
L.reff_quantizer_search.argtypes = [P, I64, P, I64, P, P]
L.reff_search_preassigned.argtypes = [P, I64, P, I64, I64, P, P, C.c_int, P, P]
L.reff_set_threads.argtypes = [C.c_int]


def p(a):
    return a.ctypes.data_as(P) if a is not None else None


def ok(rc):
    if rc != 0:
        raise RuntimeError(L.reff_last_error().decode())


def preassigned(h, c, k, store_pairs=0):
    D = np.empty((sd.NQ, k), np.float32)
    I = np.empty((sd.NQ, k), np.int64)
    ok(L.reff_search_preassigned(h, sd.NQ, p(c["xq"]), k, c["nlist"], p(c["keys"]), p(c["cdis"]),
                                 store_pairs, p(D), p(I)))
    return D, I


def with_params(h, c, k, max_codes, sel):
    D = np.empty((sd.NQ, k), np.float32)
    I = np.empty((sd.NQ, k), np.int64)
    ok(L.reff_search_params(h, sd.NQ, p(c["xq"]), k, c["nlist"], max_codes, p(sel),
                            0 if sel is None else sel.size, p(D), p(I)))
    return D, I


def main():
    os.makedirs(OUTD, exist_ok=True)
    float_rand = ge.load_oracle().float_rand
    L.reff_set_threads(1)
    fx = {}
    for tag in sd.TAGS:
        c = sd.make(float_rand, tag)
        d, nb, nlist = c["d"], c["nb"], c["nlist"]
        with tempfile.TemporaryDirectory() as tmp:
            f0 = os.path.join(tmp, "empty.faiss")
            with open(f0, "wb") as f:
                f.write(sd.empty_iwsq(d, c["qtype"], c["l2"], c["by_residual"], c["cent"],
                                      c["trained"]))
            h = L.reff_read_index(f0.encode(), 0)
        if not h:
            raise RuntimeError(L.reff_last_error().decode())
        ids = np.random.RandomState(sd.seed_of(tag)).permutation(nb).astype(np.int64) * 5 + 1
        ok(L.reff_add_core(h, nb, p(c["xb"]), p(ids), p(c["lists"])))
        ok(L.reff_write_index(h, os.path.join(OUTD, tag + ".faiss").encode()))
        # [d, nlist, nb, qtype, metric_l2, by_residual, seed]
        fx[f"{tag}_meta"] = np.array([d, nlist, nb, c["qtype"], c["l2"], c["by_residual"],
                                      sd.seed_of(tag)], np.int64)
        fx[f"{tag}_xb_sha"] = sd.sha(c["xb"])
        fx[f"{tag}_ids"] = ids.astype(np.int32)
        fx[f"{tag}_xq"], fx[f"{tag}_keys"], fx[f"{tag}_cdis"] = c["xq"], c["keys"], c["cdis"]
        for k in (1, 10, 600, 2 * nb):
            D, I = preassigned(h, c, k)
            fx[f"{tag}_pre_{k}_D"], fx[f"{tag}_pre_{k}_I"] = D, I.astype(np.int32)
        if tag in sd.PARAM_TAGS:
            D, I = preassigned(h, c, 10, store_pairs=1)
            fx[f"{tag}_sp_10_D"], fx[f"{tag}_sp_10_I"] = D, I  # list << 32 | offset: int64
            Dq = np.empty((sd.NQ, nlist), np.float32)
            Iq = np.empty((sd.NQ, nlist), np.int64)
            ok(L.reff_quantizer_search(h, sd.NQ, p(c["xq"]), nlist, p(Dq), p(Iq)))
            fx[f"{tag}_q_D"], fx[f"{tag}_q_I"] = Dq, Iq
            sel = np.ascontiguousarray(np.sort(ids)[::2])
            for mc in sd.MAX_CODES:
                D, I = with_params(h, c, 10, mc, None)
                fx[f"{tag}_params_mc{mc}_D"], fx[f"{tag}_params_mc{mc}_I"] = D, I.astype(np.int32)
            D, I = with_params(h, c, 10, 0, sel)
            fx[f"{tag}_params_sel_D"], fx[f"{tag}_params_sel_I"] = D, I.astype(np.int32)
            D, I = with_params(h, c, 10, 300, sel)
            fx[f"{tag}_params_mc300_sel_D"], fx[f"{tag}_params_mc300_sel_I"] = D, I.astype(np.int32)
        L.reff_free(h)
    np.savez_compressed(OUT, **fx)
    tot = os.path.getsize(OUT)
    print(f"{OUT}: {tot} bytes")
    for tag in sd.TAGS:
        f = os.path.join(OUTD, tag + ".faiss")
        print(f"{f}: {os.path.getsize(f)} bytes")
        tot += os.path.getsize(f)
    print(f"total {tot} bytes")


if __name__ == "__main__":
    main()
