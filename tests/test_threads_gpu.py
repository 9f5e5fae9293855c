"""The engine handle is shared by the agent's worker threads (the reference's connection pool allows 10 concurrent
`DocumentStore.search` calls, /root/reference/database/connection.py:38-42): every C-ABI entry takes the handle's mutex, so
concurrent host-pointer calls on ONE handle must return exactly what the same calls return one after the other (ctypes
releases the GIL during a call, so the threads really are inside the library at the same time)."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_concurrent_host_calls_on_one_handle_match_the_serial_results():
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.bm25 import Bm25Postings
    rng = np.random.default_rng(10)
    N, D, T = 30000, 1536, 8
    emb = rng.standard_normal((N, D)).astype(np.float32)
    eng = RagEngine(dim=D, device=0)
    try:
        eng.index_load(emb)
        docs = [" ".join(f"t{t}" for t in rng.integers(0, 800, 20)) for _ in range(N)]
        post = Bm25Postings.from_corpus(docs).load(eng)
        work = []
        for t in range(T):
            q = (emb[rng.integers(0, N, 3)] + 0.3 * rng.standard_normal((3, D))).astype(np.float32)
            ptr, terms = post.encode_queries([docs[int(rng.integers(0, N))] for _ in range(3)])
            a = rng.standard_normal((5 + t, D)).astype(np.float32)
            work.append((q, ptr, terms, a))

        def calls(item):
            q, ptr, terms, a = item
            ids, rows, sc = eng.dense_topk(q, 7 + len(a) % 3)
            b_ids, _, b_sc, _ = eng.bm25_topk(ptr, terms, 10)
            return ids.copy(), sc.copy(), b_ids.copy(), b_sc.copy(), eng.pairwise_cosine(a).copy()

        serial = [calls(w) for w in work]
        out, errs = [None] * T, []

        def worker(i):
            try:
                for _ in range(6):                      # several rounds: the threads keep colliding inside the library
                    out[i] = calls(work[i])
            except Exception as e:                       # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=worker, args=(i,)) for i in range(T)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for got, exp in zip(out, serial):
            for g, e in zip(got, exp):
                np.testing.assert_array_equal(g, e)
    finally:
        eng.close()


def test_host_calls_from_two_threads_while_a_third_feeds_a_stream_with_device_searches():
    """One thread keeps a side stream fed with device-pointer searches of the handle while two others make host calls on it
    (include/rag_hip.h, "Ordering": a host call may be made while device-pointer work of the handle is pending). Every
    result, device side and host side, equals the serial one."""
    import torch
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.bm25 import Bm25Postings
    rng = np.random.default_rng(12)
    N, D, Q, k, rounds = 30000, 256, 300, 20, 12
    emb = rng.standard_normal((N, D)).astype(np.float32)
    docs = [" ".join(f"t{t}" for t in rng.integers(0, 500, 12)) for _ in range(N)]
    eng = RagEngine(dim=D, device=0)
    try:
        eng.index_load(emb)
        post = Bm25Postings.from_corpus(docs).load(eng)
        batches = [(emb[rng.integers(0, N, Q)] + 0.3 * rng.standard_normal((Q, D))).astype(np.float32) for _ in range(3)]
        host_q = [(emb[rng.integers(0, N, 1 + i)] + 0.3 * rng.standard_normal((1 + i, D))).astype(np.float32) for i in range(2)]
        host_t = [post.encode_queries([docs[int(rng.integers(0, N))]]) for _ in range(2)]
        small = [rng.standard_normal((6 + i, D)).astype(np.float32) for i in range(2)]

        def host_calls(i):
            ids, _, sc = eng.dense_topk(host_q[i], 5 + i)
            b_ids, _, b_sc, _ = eng.bm25_topk(host_t[i][0], host_t[i][1], 10)
            return ids.copy(), sc.copy(), b_ids.copy(), b_sc.copy(), eng.pairwise_cosine(small[i]).copy()

        dev_ref = [eng.dense_topk(b, k) for b in batches]
        host_ref = [host_calls(i) for i in range(2)]
        s = torch.cuda.Stream()
        qd = [torch.from_numpy(b).cuda() for b in batches]
        torch.cuda.synchronize()
        dev_out, host_out, errs = [], [[], []], []

        def feeder():
            try:
                with torch.cuda.stream(s):
                    for r in range(rounds):
                        ids = torch.empty((Q, k), dtype=torch.int64, device="cuda")
                        rows = torch.empty((Q, k), dtype=torch.int32, device="cuda")
                        sc = torch.empty((Q, k), dtype=torch.float64, device="cuda")
                        eng.dense_topk_dev(qd[r % 3], k, ids, rows, sc, stream=s)
                        dev_out.append((r % 3, ids, rows, sc))
            except Exception as e:                       # noqa: BLE001
                errs.append(e)

        def host_worker(i):
            try:
                for _ in range(6):
                    host_out[i].append(host_calls(i))
            except Exception as e:                       # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=feeder)] + [threading.Thread(target=host_worker, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        s.synchronize()
        assert not errs, errs
        assert len(dev_out) == rounds
        for b, ids, rows, sc in dev_out:
            for g, e in zip((ids, rows, sc), dev_ref[b]):
                np.testing.assert_array_equal(g.cpu().numpy(), e)
        for i in range(2):
            assert len(host_out[i]) == 6
            for got in host_out[i]:
                for g, e in zip(got, host_ref[i]):
                    np.testing.assert_array_equal(g, e)
    finally:
        eng.close()
