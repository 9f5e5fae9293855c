"""GPU: GpuDocumentIndex live writes on a real engine - a shard loaded with headroom, document ids from the shard,
add_rows / archival inserts / document chunks / deletes / compaction over _ShardRows, checked against a pure-Python model of
the SQL table (exact float64 cosine, WHERE agent_id, ORDER BY, LIMIT), and a concurrent search that never sees a half-replaced
document."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 128


def model_search(table, agent, q, limit):
    q = np.asarray(q, np.float32).astype(np.float64)
    rows = [r for r in table if r["agent_id"] == agent]
    sims = [float(q @ e / (np.linalg.norm(q) * np.linalg.norm(e))) for e in (np.asarray(r["emb"], np.float64) for r in rows)]
    return [rows[i]["content"] for i in sorted(range(len(rows)), key=lambda i: -sims[i])[:limit]]


def write_shard(path, rng, n, with_doc_ids):
    from optimized_rag_amd import shard_format as SF
    w = SF.ShardWriter(path, dim=D)
    table = []
    for i in range(n):
        e = rng.standard_normal(D).astype(np.float32)
        agent, doc = f"a{i % 3}", (i // 6 if with_doc_ids else None)
        w.add(1000 + i, agent, f"s{i}", e, document_id=doc)
        table.append({"id": 1000 + i, "agent_id": agent, "content": f"s{i}", "emb": e, "document_id": doc})
    w.close(build_bm25=False)
    return table


def test_shard_with_headroom_live_writes_vs_sql_model(tmp_path):
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.document_store import GpuDocumentIndex
    rng = np.random.default_rng(0)
    table = write_shard(str(tmp_path / "s"), rng, 120, True)
    eng = RagEngine(dim=D, device=0)
    try:
        idx = GpuDocumentIndex(None, dim=D, engine=eng)
        idx.load_shard(str(tmp_path / "s"), headroom_rows=64)
        for step in range(12):
            agent = f"a{step % 3}"
            if step % 4 == 0:
                e = rng.standard_normal(D).astype(np.float32)
                mid = idx.insert_archival_memory(agent, f"m{step}", e.tolist(), {"k": step})
                table.append({"id": mid, "agent_id": agent, "content": f"m{step}", "emb": e, "document_id": None})
            elif step % 4 == 1:
                doc = int(rng.integers(0, 20))
                owner = next((r["agent_id"] for r in table if r["document_id"] == doc), agent)
                assert idx.delete_document(owner, doc) is True
                table = [r for r in table if not (r["document_id"] == doc and r["agent_id"] == owner)]
            elif step % 4 == 2:
                embs = rng.standard_normal((3, D)).astype(np.float32)
                res = idx.index_document_chunks(agent, 500 + step, [{"content": f"c{step}.{j}"} for j in range(3)], embs.tolist())
                assert res["chunks_created"] == 3
                table += [{"agent_id": agent, "content": f"c{step}.{j}", "emb": embs[j], "document_id": 500 + step} for j in range(3)]
            else:
                idx.compact()                                  # remaps _ShardRows + appended rows
            q = rng.standard_normal(D)
            for a in ("a0", "a1", "a2"):
                got = [h["content"] for h in idx.search_archival_memory(a, q.tolist(), limit=9)]
                assert got == model_search(table, a, q, 9)
    finally:
        eng.close()


def test_shard_without_document_ids_cannot_delete_documents(tmp_path):
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.document_store import GpuDocumentIndex
    rng = np.random.default_rng(1)
    write_shard(str(tmp_path / "s"), rng, 30, False)
    eng = RagEngine(dim=D, device=0)
    try:
        idx = GpuDocumentIndex(None, dim=D, engine=eng)
        idx.load_shard(str(tmp_path / "s"))
        assert idx.delete_document("a0", 0) is False
    finally:
        eng.close()


def test_concurrent_search_never_sees_a_half_replaced_document():
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.document_store import GpuDocumentIndex
    rng = np.random.default_rng(2)
    eng = RagEngine(dim=D, device=0)
    try:
        idx = GpuDocumentIndex(None, dim=D, engine=eng)
        other = rng.standard_normal((50, D)).astype(np.float32)
        idx.bulk_load([{"content": f"o{i}", "agent_id": "other"} for i in range(50)], other)
        sets = {s: rng.standard_normal((4, D)).astype(np.float32) for s in "AB"}
        idx.index_document_chunks("x", 1, [{"content": f"A{j}"} for j in range(4)], sets["A"].tolist())
        stop, seen, bad = threading.Event(), [], []

        def writer():
            for i in range(40):
                s = "B" if i % 2 == 0 else "A"
                idx.index_document_chunks("x", 1, [{"content": f"{s}{j}"} for j in range(4)], sets[s].tolist())
            stop.set()

        def reader():
            q = rng.standard_normal(D).tolist()
            while not stop.is_set():
                got = sorted(h["content"] for h in idx.search_archival_memory("x", q, limit=10))
                seen.append(got)
                if got not in (sorted(f"A{j}" for j in range(4)), sorted(f"B{j}" for j in range(4))):
                    bad.append(got)

        ts = [threading.Thread(target=writer), threading.Thread(target=reader), threading.Thread(target=reader)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=120)
        assert seen and not bad, bad[:3]
    finally:
        eng.close()
