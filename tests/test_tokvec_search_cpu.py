"""CPU: what the exhaustive MaxSim search (mode 2 of rag_retrieve_maxsim_dev) must hold without a GPU. It adds no exported symbol -
the header still declares exactly _lib.exported_symbols() - the Python layers have their new methods, and the truth helper of
tests/tokvec_search_tools.py agrees with a plain double loop on a 12-document world. (rag_set_option needs a handle, and a handle
needs a GPU: the two option names are checked in tests/test_tokvec_search_gpu.py.)"""
import inspect
import os
import re

import numpy as np

import tokvec_search_tools as W

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_header_declares_exactly_the_exported_symbols():
    from optimized_rag_amd import _lib
    declared = set(re.findall(r"\b(rag_[a-z0-9_]+)\s*\(", read("include", "rag_hip.h")))
    assert declared == set(_lib.exported_symbols())


def test_the_header_and_the_option_table_name_mode_2_and_its_options():
    header, api = read("include", "rag_hip.h"), read("optimized-rag_amd", "csrc", "api.hip")
    for name in ("tokvec_scan_ws_mb", "tokvec_scan_queries"):
        assert name in header and f'{{"{name}", &rag_options::{name}}}' in api
    assert "mode 2, the exhaustive MaxSim search" in header and "BIT-IDENTITY" in header


def test_the_python_layers_have_the_search():
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.document_store import GpuDocumentIndex
    from optimized_rag_amd.sharded import ShardedM3Index
    assert list(inspect.signature(RagEngine.tokvec_search_dev).parameters) == ["self", "q_vecs", "q_off", "k", "pool", "tenant", "stream"]
    assert list(inspect.signature(ShardedM3Index.search_maxsim).parameters) == ["self", "q_vecs", "q_off", "k", "tenant"]
    assert '"maxsim"' in inspect.getsource(GpuDocumentIndex.search_late_interaction)


def test_the_world_is_the_one_the_issue_describes():
    for dim in W.DIMS:
        w = W.world(dim)
        counts = np.diff(w["off"])
        assert counts.shape == (W.N_DOCS,) and counts[:12].tolist() == list(W.EDGE_ROWS) and 1 <= counts[36:].min() and counts.max() == 255
        assert np.diff(w["qo"]).tolist() == list(W.Q_ROWS) and w["vecs"].shape == (int(w["off"][-1]), dim)
        src = w["vecs"][w["off"][W.SRC]:w["off"][W.SRC + 1]]
        for c in W.COPIES:
            np.testing.assert_array_equal(w["vecs"][w["off"][c]:w["off"][c + 1]], src)
        assert W.COPIES[1] == W.N_DOCS - 1 and W.PER_QUERY.tolist() == [-1, 0, 1, 2, -1, 0, 1, 2, -1]
    assert W.slices(700) == [(0, 256), (256, 256), (512, 188)]


def test_the_truth_helper_agrees_with_a_double_loop():
    rng = np.random.default_rng(4)
    q_off = np.array([0, 3, 3, 8, 9], dtype=np.int64)                   # query 1 has no rows
    d_off = np.concatenate([[0], np.cumsum([2, 0, 5, 1, 7, 3, 3, 0, 4, 6, 2, 9])]).astype(np.int64)
    tenants = (np.arange(12) % 3).astype(np.int32)
    scores = rng.integers(0, 4, (4, 12)).astype(np.float32) / 4         # few values: many exact ties
    scores[:, [1, 7]] = 0
    for q_tenants in (-1, 2, np.array([-1, 0, 1, 2])):
        mask = W.ranked(q_off, d_off, tenants, (5, 11), q_tenants)
        assert not mask[1].any() and not mask[:, [1, 5, 7, 11]].any() and mask[0].sum() == (8 if np.ndim(q_tenants) or q_tenants < 0 else 2)
        for pool, k in ((5, 3), (12, 12), (1, 1), (20, 4)):
            got, exp = W.truth(scores, mask, pool, k), W.truth_loops(scores, mask, pool, k)
            for g, x in zip(got, exp):
                np.testing.assert_array_equal(g, x)
    ids = 100 + 7 * np.arange(12)
    mask = W.ranked(q_off, d_off, tenants, (), -1)
    a, b = W.truth(scores, mask, 6, 2, ids=ids), W.truth(scores, mask, 6, 2)
    np.testing.assert_array_equal(a[0], np.where(b[0] >= 0, 100 + 7 * b[0], -1))
    np.testing.assert_array_equal(a[2], np.where(b[2] >= 0, 100 + 7 * b[2], -1))
