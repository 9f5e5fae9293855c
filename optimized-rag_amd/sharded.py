"""Row-sharded search across the GPUs of one node: one process per GPU, corpus rows (embeddings, BM25
postings, token ids) partitioned contiguously, ONE small collective per stage.

    dense :  local top-k (rag_dense_topk_dev)  ->  all_gather of [ids | float64 score bits]  ->  rag_merge_topk_dev
    hybrid:  local dense top-pool + local RAW BM25 top-pool (global idf / avgdl replicated)  ->  ONE all_gather of both
             lists  ->  rag_hybrid_fuse_gathered_dev: two merges, BM25 / global max, RRF on the MERGED lists (RRF needs
             GLOBAL ranks, so the lists are merged before fusing) - all inside the library
    linear:  every document's raw BM25 score + the local maximum (rag_hybrid_linear_begin_dev)  ->  all_gather of [Q] float64 maxima
             ->  the fused search under the GLOBAL maximum (rag_hybrid_linear_finish_dev)  ->  all_gather of [5][Q][k] blocks  ->
             rag_hybrid_linear_merge_gathered_dev (hybrid desc, id asc, components carried): ShardedHybridIndex.search_linear
    bge-m3:  local dense + sparse top-pool  ->  all_gather  ->  rag_m3_candidates_gathered_dev (merges, RRF on the merged lists)
             ->  rag_m3_score_ids_dev (the rank that holds a candidate's rows and token vectors scores it)  ->  all_gather  ->
             rag_m3_combine_gathered_dev (owner select, three-way combine, stable top-k): ShardedM3Index
    rerank:  the Q x pool pairs are independent: each rank scores a contiguous slice (rag_ce_score_dev), one all_gather
             of the logits

The reference is single-process (no collective to mirror). torch.distributed (backend "nccl" = RCCL over xGMI on
the GPU box, "gloo" in CPU tests) is plumbing only (buffers, process group, the gather itself unless engine.comm_init
bound RCCL behind the C-ABI); every piece of arithmetic on the gathered lists is a HIP kernel of the library. The payload is Q*k*16 B per rank
(327 KB at Q=1024, k=20): latency-bound, so one fused gather of both arrays rather than two collectives.
"""
import numpy as np
import torch
import torch.distributed as dist

from ._lib import _tenant_arg
from .bm25 import Bm25Postings


def shard_bounds(n_rows, world):
    """Contiguous row ranges [begin, end) per rank; the first n_rows % world ranks get one extra row."""
    base, extra = divmod(int(n_rows), int(world))
    out, b = [], 0
    for r in range(world):
        e = b + base + (1 if r < extra else 0)
        out.append((b, e))
        b = e
    return out


class ShardedDenseIndex:
    def __init__(self, engine, rank=None, world=None, group=None):
        self.engine = engine
        self.group = group
        self.world = world if world is not None else (dist.get_world_size(group) if dist.is_initialized() else 1)
        self.rank = rank if rank is not None else (dist.get_rank(group) if dist.is_initialized() else 0)
        self._bufs = {}

    def load_shard(self, emb_shard, first_global_row, ids=None):
        """emb_shard: this rank's rows; doc ids become first_global_row + local row. With `ids` (int64, one per row, strictly
        ascending - else ValueError) the shard stores them as explicit ids and enables the device id-to-row map
        (RagEngine.index_id_map): such a shard takes the writes below, and first_global_row is not used."""
        if ids is None:
            self.engine.index_load(emb_shard, id_base=int(first_global_row))
            self._explicit = False
            self._local_max_id = int(first_global_row) + int(emb_shard.shape[0]) - 1
        else:
            ids = np.ascontiguousarray(ids, dtype=np.int64)
            if ids.shape != (emb_shard.shape[0],) or (ids.size and int(ids[0]) < 0) or not (np.diff(ids) > 0).all():
                raise ValueError("load_shard: ids must be one id >= 0 per row, strictly ascending on the shard")
            self.engine.index_load(emb_shard, ids=ids)
            self.engine.index_id_map(True)
            self._explicit = True
            self._local_max_id = int(ids[-1]) if ids.size else -1
        self._layout = None

    # ---- writes on shards. SPMD calls, like the searches: every rank makes the same call with the same arguments. What every
    # rank knows about the others is one small record, the LAYOUT: each rank's row count, the largest id anywhere and the number
    # of keyword terms known anywhere. It is agreed by one gather of three int64 per rank at the first write after a load and
    # after compact(); in between every rank updates its copy by the same rule, with no collective. local_layout / agree_layout
    # are the halves on each side of that gather, so that one process can stand in for several ranks.
    def _local_terms(self):
        return 0

    def _rows_changed(self):
        """A write changed this rank's or another rank's row count (a hook for what a subclass agreed on from the counts)."""

    def local_layout(self):
        """This rank's share of the layout: [rows, largest id (-1 without rows), keyword terms known]."""
        return [int(self.engine.n_rows), int(self._local_max_id), int(self._local_terms())]

    def agree_layout(self, all_layouts):
        """all_layouts: every rank's local_layout(), in rank order."""
        if len(all_layouts) != self.world:
            raise ValueError(f"agree_layout: expected {self.world} layouts, got {len(all_layouts)}")
        self._layout = dict(rows=[int(l[0]) for l in all_layouts], max_id=max(int(l[1]) for l in all_layouts),
                            terms=max(int(l[2]) for l in all_layouts))
        return self._layout

    def _gather_numbers(self, mine):
        """[world, len(mine)] int64 on the host: one gather of a few numbers per rank."""
        if self.world == 1:
            return [list(mine)]
        dev = torch.device("cuda", self.engine.device)
        send = torch.tensor(list(mine), dtype=torch.int64, device=dev)
        recv = torch.empty((self.world, send.shape[0]), dtype=torch.int64, device=dev)
        _gather(recv, send, self.group, self.engine)
        return recv.tolist()

    def layout(self):
        if getattr(self, "_layout", None) is None:
            self.agree_layout(self._gather_numbers(self.local_layout()))
        return self._layout

    @staticmethod
    def owner_of(rows_per_rank):
        """The owner policy: the rank with the fewest rows, ties to the lowest rank. A function of the layout alone."""
        rows = [int(r) for r in rows_per_rank]
        return rows.index(min(rows))

    def _check_block(self, emb, ids, owner):
        """What must hold before ANY rank changes anything -> (ids int64, owner, the owner's first new row)."""
        if not getattr(self, "_explicit", False):
            raise ValueError("insert_rows: the shard was loaded without ids (load_shard(..., ids=...))")
        lay = self.layout()
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int64)
        n = int(np.asarray(emb).shape[0]) if np.ndim(emb) == 2 else 1
        if ids.shape != (n,) or n == 0:
            raise ValueError(f"insert_rows: need one id per row, got {ids.shape} for {n} rows")
        if not (np.diff(ids) > 0).all():
            raise ValueError("insert_rows: ids must be strictly ascending")
        if int(ids[0]) <= lay["max_id"]:
            raise ValueError(f"insert_rows: ids must be above the largest id of the index, {lay['max_id']} (got {int(ids[0])})")
        if owner is None:
            owner = self.owner_of(lay["rows"])
        if not 0 <= int(owner) < self.world:
            raise ValueError(f"insert_rows: owner {owner} is no rank of {self.world}")
        return ids, int(owner), lay["rows"][int(owner)]

    def _block_done(self, ids, owner, n_terms_total=None):
        lay = self._layout
        lay["rows"][owner] += int(ids.shape[0])
        lay["max_id"] = int(ids[-1])
        if n_terms_total is not None:
            lay["terms"] = max(lay["terms"], int(n_terms_total))
        if owner == self.rank:
            self._local_max_id = int(ids[-1])
        self._rows_changed()

    def insert_rows(self, emb, ids, tenants=None, temporal=None, owner=None):
        """A block of new rows (host arrays, replicated): ids strictly ascending and above every id of the index - a BIGSERIAL
        key - else ValueError before any rank changes anything; so no id can exist twice across shards, without a lookup. The
        whole block goes to ONE rank: `owner`, or the rank with the fewest rows (ties: the lowest rank), which every rank
        computes from its copy of the layout. The owner inserts, the others update the layout. Returns (owner, the block's first
        row on the owner)."""
        ids, owner, first = self._check_block(emb, ids, owner)
        if owner == self.rank:
            got = self.engine.index_insert(emb, ids=ids, tenants=tenants, temporal=temporal)
            assert got == first, (got, first)
        self._block_done(ids, owner)
        return owner, first

    def delete_local(self, ids, tenant=-1):
        """This rank's half of delete_ids: the rows it holds of these ids (and of `tenant`, when >= 0) -> their number."""
        return self.engine.index_delete(ids, tenant=tenant)

    def delete_ids(self, ids, tenant=-1):
        """Every rank deletes what it holds of these ids; returns the number of rows deleted anywhere (one gather of one number)."""
        mine = self.delete_local(ids, tenant)
        return sum(int(r[0]) for r in self._gather_numbers([mine]))

    def compact_local(self):
        """This rank's half of compact(): the local compaction with postings and resident data kept -> its row map."""
        row_map = self.engine.index_compact(keep_resident=True)
        self._layout = None
        self._rows_changed()
        return row_map

    def compact(self):
        """Every rank removes its deleted rows (rag_index_compact_live: BM25 and learned-sparse postings and the token vectors
        move with the rows), then the layout is agreed again. Ids do not change, so no other rank is affected. Returns this
        rank's row map."""
        row_map = self.compact_local()
        self.layout()
        return row_map

    def _buffers(self, Q, k, device):
        key = (Q, k, str(device))
        b = self._bufs.get(key)
        if b is None:
            send = torch.empty((2, Q, k), dtype=torch.int64, device=device)
            recv = torch.empty((self.world, 2, Q, k), dtype=torch.int64, device=device)
            out_ids = torch.empty((Q, k), dtype=torch.int64, device=device)
            out_scores = torch.empty((Q, k), dtype=torch.float64, device=device)
            # views are made once: search() is on the per-batch path (0.6 ms per batch on an 8-way shard of 1M rows)
            b = self._bufs[key] = (send, recv, out_ids, out_scores, send[0], send[1].view(torch.float64),
                                   recv.view(torch.float64)[:, 1])
        return b

    def search(self, queries, k, tenant=-1):
        """queries: [Q, dim] float32 tensor replicated on every rank. Returns (ids [Q,k] int64, scores [Q,k] f64)
        of the GLOBAL top-k on every rank: cosine desc, lower doc id first on ties."""
        Q = queries.shape[0]
        send, recv, out_ids, out_scores, send_ids, send_sc, recv_sc = self._buffers(Q, k, queries.device)
        self.engine.dense_topk_dev(queries, k, send_ids, None, send_sc, tenant=tenant)
        if self.world == 1:
            return send_ids, send_sc
        _gather(recv, send, self.group, self.engine)
        self.engine.merge_topk_dev(recv, recv_sc, out_ids, out_scores, n_lists=self.world, list_stride=2 * Q * k)
        return out_ids, out_scores


def _gather(recv, send, group, engine=None):
    if engine is not None and getattr(engine, "comm_world", 0) > 1:     # RCCL bound behind the C-ABI (engine.comm_init ran)
        engine.comm_allgather_dev(send, recv)
    elif dist.get_backend(group) == "nccl":                 # RCCL: one flat gather straight into the merge buffer
        dist.all_gather_into_tensor(recv, send, group=group)
    else:
        dist.all_gather(list(recv.unbind(0)), send, group=group)


class ShardedHybridIndex(ShardedDenseIndex):
    """Dense + BM25 + RRF over row shards. Every rank ends up with the same global result.

    The engine of each rank holds its rows of the embedding matrix (ids = first_global_row + local row) and the
    doc-partitioned slice of the postings built by Bm25Postings.shard (global statistics), loaded row-aligned so both
    searches speak the same doc-id space."""

    # search_linear: queries per begin / finish pair. None = the smallest hybrid_linear_batch() of the ranks, agreed once per
    # load; a number (the SAME on every rank, not above that) forces smaller pieces.
    linear_sub_batch = None

    def load_shard(self, emb_shard, first_global_row, postings_shard=None, temporal=None, ids=None):
        """temporal: this rank's slice of the per-row temporal vector of search_linear (float64 [rows]; None = zeros).
        ids: ShardedDenseIndex.load_shard."""
        super().load_shard(emb_shard, first_global_row, ids=ids)
        self._idf = None
        if postings_shard is not None:
            postings_shard.load(self.engine)
            # the GLOBAL idf table (replicated at the load, grown by every insert_rows on every rank, replaced by
            # refresh_statistics): a later block's owner takes from it the idf of terms that other ranks' blocks introduced
            self._idf = np.array(postings_shard.idf, dtype=np.float64)
            self._epsilon = float(getattr(postings_shard, "epsilon", 0.25))
        self.engine.bm25_set_normalize(False)
        if temporal is not None or getattr(self, "_has_temporal", False):      # (None after a vector clears it: a reload keeps none)
            self.engine.set_temporal(temporal)
            self._has_temporal = temporal is not None
        self._lin_agreed = None

    def _rows_changed(self):
        self._lin_agreed = None                 # the sub-batch of search_linear follows the row counts: agreed again at the next search

    def _local_terms(self):
        return 0 if getattr(self, "_idf", None) is None else int(self.engine.bm25_segment_stats()["n_terms"])

    def insert_rows(self, emb, ids, tenants=None, temporal=None, owner=None, postings=None):
        """ShardedDenseIndex.insert_rows with the block's BM25 postings: `postings` is what Bm25Postings.extend returned for the
        block's texts on the mirror of the WHOLE corpus (CSR over the grown global vocabulary, documents relative to the block,
        idf_new of the terms the block introduced). The owner appends them (rag_bm25_append_host) with the idf of every term ITS
        handle does not know yet - those of this block and those that blocks of other ranks introduced, from the recorded table.
        A rank that never sees a term needs nothing: a query term past a handle's vocabulary is out of vocabulary there."""
        ids, owner, first = self._check_block(emb, ids, owner)
        V = None
        if postings is not None:
            if self._idf is None:
                raise ValueError("insert_rows: postings given but the shard was loaded without any")
            V, idf_new = int(postings["n_terms_total"]), np.asarray(postings["idf_new"], dtype=np.float64)
            if V != self._idf.shape[0] + idf_new.shape[0] or self._idf.shape[0] != self.layout()["terms"]:
                raise ValueError(f"insert_rows: the block counts {V} terms with {idf_new.shape[0]} new ones, the index knows {self._idf.shape[0]}")
        elif self._idf is not None:
            raise ValueError("insert_rows: the shard has BM25 postings: the block's postings are required")
        if owner == self.rank:
            got = self.engine.index_insert(emb, ids=ids, tenants=tenants, temporal=temporal)
            assert got == first, (got, first)
        if postings is not None:
            self._idf = np.concatenate([self._idf, idf_new])
            if owner == self.rank:
                known = self._local_terms()
                self.engine.bm25_append(postings["indptr"], postings["doc"], postings["tf"], postings["doc_len"], self._idf[known:V], V)
        self._block_done(ids, owner, V)
        return owner, first

    def local_statistics(self):
        """This rank's half of refresh_statistics: int64 [global terms + 2] = df of every term over its live documents (0 for a
        term its handle does not know) | live documents | the sum of their lengths."""
        df, n, total = self.engine.bm25_live_counts()
        out = np.zeros(self.layout()["terms"] + 2, dtype=np.int64)
        out[:df.shape[0]] = df
        out[-2:] = (n, total)
        return out

    def apply_statistics(self, all_statistics, epsilon=None):
        """all_statistics: every rank's local_statistics(). Integer sums, so exact; then the idf rule of rag_bm25_refresh on the
        host (Bm25Postings.idf_of_counts) and rag_bm25_set_statistics_host with this handle's prefix of the table."""
        tot = np.sum(np.asarray(all_statistics, dtype=np.int64), axis=0)
        n, length = int(tot[-2]), int(tot[-1])
        if n == 0:
            raise ValueError("refresh_statistics: no live document on any rank")
        eps = self._epsilon if epsilon is None else float(epsilon)
        self._idf, _ = Bm25Postings.idf_of_counts(tot[:-2], n, eps)
        avgdl = length / n
        self.engine.bm25_set_statistics(self._idf[:self._local_terms()], avgdl)
        return self._idf, avgdl

    def refresh_statistics(self, epsilon=0.25):
        """idf and avgdl over the live documents of EVERY shard, as rag_bm25_refresh computes them on the unsharded index: one
        gather of (terms + 2) int64 per rank. Needs option bm25_keep_tf set before the postings were loaded. Returns (idf of
        every known term, avgdl)."""
        mine = self.local_statistics()
        return self.apply_statistics(self._gather_numbers(mine.tolist()), epsilon)

    def _hyb_buffers(self, Q, pool, k, device):
        key = ("hyb", Q, pool, k, str(device))
        if key not in self._bufs:
            i64, f64 = torch.int64, torch.float64
            self._bufs[key] = dict(
                send=torch.empty((4, Q, pool), dtype=i64, device=device),          # dense ids | dense score bits | bm25 ids | bm25 raw bits
                recv=torch.empty((self.world, 4, Q, pool), dtype=i64, device=device),
                lists=torch.empty((2, Q, pool), dtype=i64, device=device),         # merged dense ids | merged BM25 ids
                scores=torch.empty((2, Q, pool), dtype=f64, device=device),        # cosines | BM25 / global max
                keys=torch.empty((Q, k), dtype=i64, device=device),
                rrf=torch.empty((Q, k), dtype=f64, device=device),
                ranks=torch.empty((Q, k, 2), dtype=torch.int32, device=device))
        return self._bufs[key]

    def local_lists(self, queries, term_ptr, terms, pool, k, tenant=-1):
        """This rank's half of the exchange: [4, Q, pool] int64 = dense ids | dense score bits | BM25 ids | raw BM25 bits."""
        send = self._hyb_buffers(queries.shape[0], pool, k, queries.device)["send"]
        f64 = torch.float64
        self.engine.dense_topk_dev(queries, pool, send[0], None, send[1].view(f64), tenant=tenant)
        self.engine.bm25_topk_dev(term_ptr, terms, pool, send[2], None, send[3].view(f64), tenant=tenant)
        return send

    def fuse_gathered(self, recv, k, rrf_k=60):
        """recv: [world, 4, Q, pool] int64, every rank's local_lists() -> the global result (see search_hybrid)."""
        world, _, Q, pool = recv.shape
        b = self._hyb_buffers(Q, pool, k, recv.device)
        # two merges, BM25 / global max (rag/retrieval.py:343-345), RRF on the merged lists: one library call, no torch arithmetic
        self.engine.hybrid_fuse_gathered_dev(recv, k, b["lists"], b["scores"], b["keys"], b["rrf"], b["ranks"], rrf_k=rrf_k)
        return dict(keys=b["keys"], rrf=b["rrf"], ranks=b["ranks"], dense_ids=b["lists"][0], dense_scores=b["scores"][0],
                    bm25_ids=b["lists"][1], bm25_scores=b["scores"][1])

    def search_hybrid(self, queries, term_ptr, terms, pool, k, rrf_k=60, tenant=-1):
        """queries [Q, dim] float32, term_ptr [Q+1] / terms int32 (global term ids, -1 = unknown), all replicated.
        Returns dict(keys [Q,k], rrf [Q,k], ranks [Q,k,2] (1-based rank in the dense / BM25 list, 0 = absent),
        dense_ids/dense_scores [Q,pool], bm25_ids/bm25_scores [Q,pool] (scores max-normalised with the GLOBAL max))."""
        send = self.local_lists(queries, term_ptr, terms, pool, k, tenant)
        if self.world == 1:
            return self.fuse_gathered(send.unsqueeze(0), k, rrf_k)
        recv = self._hyb_buffers(queries.shape[0], pool, k, queries.device)["recv"]
        _gather(recv, send, self.group, self.engine)
        return self.fuse_gathered(recv, k, rrf_k)

    # ---- the reference's own fusion, (alpha * cosine + beta * BM25 / max) + gamma * temporal, over row shards ----------------
    def _lin_batch(self, device):
        """Queries per begin / finish pair, the same on every rank: agreed once per load (one gather of one number per rank)."""
        if self.linear_sub_batch is not None:
            return int(self.linear_sub_batch)
        if getattr(self, "_lin_agreed", None) is None:
            mine = self.engine.hybrid_linear_batch()
            if self.world > 1:
                send = torch.full((1,), mine, dtype=torch.int64, device=device)
                recv = torch.empty((self.world, 1), dtype=torch.int64, device=device)
                _gather(recv, send, self.group, self.engine)
                mine = min(int(v) for v in recv.flatten().tolist())
            self._lin_agreed = mine
        return self._lin_agreed

    def _lin_buffers(self, Q, k, device):
        key = ("lin", Q, k, str(device))
        if key not in self._bufs:
            i64, f64 = torch.int64, torch.float64
            self._bufs[key] = dict(mx=torch.empty((Q,), dtype=f64, device=device), mx_all=torch.empty((self.world, Q), dtype=f64, device=device),
                                   part=torch.empty((5, Q, k), dtype=i64, device=device),
                                   part_all=torch.empty((self.world, 5, Q, k), dtype=i64, device=device))
        return self._bufs[key]

    def search_linear(self, queries, term_ptr, terms, k, alpha, beta, gamma, tenant=-1):
        """HybridRetriever.hybrid_search over the row shards. queries [Q, dim] float32, term_ptr [Q+1] / terms int32 (global term
        ids), replicated; tenant an int or one number per query. Returns dict(ids [Q,k] int64, hybrid / semantic / keyword /
        temporal [Q,k] float64): the outputs of hybrid_linear_dev on the unsharded index, identical on every rank.

        Per sub-batch: hybrid_linear_begin_dev (every document's raw BM25 score, this rank's maximum)  ->  gather [world, Q]
        float64  ->  hybrid_linear_finish_dev (the fused search under the GLOBAL maximum)  ->  gather [world, 5, Q, k] int64  ->
        hybrid_linear_merge_gathered_dev. world == 1 runs the same calls without the gathers."""
        Q, dev = queries.shape[0], queries.device
        per_query, tenant = _tenant_arg(tenant, Q)
        key = ("lin_out", Q, k, str(dev))
        if key not in self._bufs:
            self._bufs[key] = dict(ids=torch.empty((Q, k), dtype=torch.int64, device=dev),
                                   **{n: torch.empty((Q, k), dtype=torch.float64, device=dev) for n in ("hybrid", "semantic", "keyword", "temporal")})
        out = self._bufs[key]
        step = self._lin_batch(dev)
        for q0 in range(0, Q, step):
            q1 = min(Q, q0 + step)
            b = self._lin_buffers(q1 - q0, k, dev)
            t = tenant[q0:q1] if per_query else tenant
            self.engine.hybrid_linear_begin_dev(term_ptr[q0:q1 + 1], terms, b["mx"], tenant=t)
            if self.world == 1:
                mx_all = b["mx"].unsqueeze(0)
            else:
                mx_all = b["mx_all"]
                _gather(mx_all, b["mx"], self.group, self.engine)
            self.engine.hybrid_linear_finish_dev(queries[q0:q1], mx_all, k, alpha, beta, gamma, b["part"], tenant=t)
            if self.world == 1:
                part_all = b["part"].unsqueeze(0)
            else:
                part_all = b["part_all"]
                _gather(part_all, b["part"], self.group, self.engine)
            self.engine.hybrid_linear_merge_gathered_dev(part_all, out["ids"][q0:q1], out["hybrid"][q0:q1], out["semantic"][q0:q1],
                                                         out["keyword"][q0:q1], out["temporal"][q0:q1])
        return out


class ShardedM3Index(ShardedDenseIndex):
    """bge-m3 over row shards: the learned-sparse list, the late-interaction rerank and the three-way score (dense + sparse +
    MaxSim), each bit-identical on every rank to the one-call entry on the unsharded index.

    Every rank holds a contiguous row range under id_base = its first global row: the embeddings, the doc-partitioned postings
    (LexicalPostings.shard) and the token vectors of its own documents. The query arrays are replicated. Two small collectives per
    batch (32 B per slot per rank each):

        local dense top-pool + local sparse top-pool  ->  gather [world, 4, Q, pool]  ->  rag_m3_candidates_gathered_dev (two
        merges, RRF on the MERGED lists)  ->  rag_m3_score_ids_dev (each rank scores the candidates whose rows it holds: their
        token vectors live nowhere else)  ->  gather [world, 4, Q, slots]  ->  rag_m3_combine_gathered_dev (owner select, combine,
        stable top-k)

    The halves on each side of each gather are methods of their own, so one process can stack the sends of several handles."""

    def load_shard(self, emb_shard, first_global_row, lexical_shard=None, token_vecs=None, token_off=None, form="fp16", ids=None,
                   token_reserve=None):
        """emb_shard: this rank's rows; lexical_shard: LexicalPostings.shard(begin, end); token_vecs [rows, dim] float32 and
        token_off [n_rows + 1] int64: the token vectors of this rank's documents, stored as `form` ("fp16" / "mxfp8").
        ids: ShardedDenseIndex.load_shard. token_reserve = (documents, token rows): room the store keeps for insert_rows beyond
        what is loaded (a store without it is full once loaded)."""
        super().load_shard(emb_shard, first_global_row, ids=ids)
        self._has_lexical = lexical_shard is not None
        self._has_tokvec = token_vecs is not None
        if lexical_shard is not None:
            lexical_shard.load(self.engine)
        if token_vecs is not None and token_reserve is None:
            self.engine.tokvec_load(token_vecs, token_off, form=form)
        elif token_vecs is not None:
            token_off = np.ascontiguousarray(token_off, dtype=np.int64)
            self.engine.tokvec_reserve(token_off.shape[0] - 1 + int(token_reserve[0]), int(token_off[-1] - token_off[0]) + int(token_reserve[1]),
                                       int(token_vecs.shape[1]), form=form)
            self.engine.tokvec_append(token_vecs, token_off)

    def insert_rows(self, emb, ids, tenants=None, temporal=None, owner=None, lexical=None, token_vecs=None, token_off=None):
        """ShardedDenseIndex.insert_rows with the block's learned-sparse postings and token vectors. lexical: what
        LexicalPostings.extend returned for the block (host CSR, documents relative to the block), or a (doc_ptr, terms, weights,
        n_terms_total) tuple of CUDA tensors, the doc-major output of lexical_compact_dev (rag_sparse_append_dev); token_vecs /
        token_off: float32 [rows, dim] and int64 [n + 1]. The owner appends both; raw sparse scores and MaxSim need no
        corpus-wide statistic, so the other ranks do nothing."""
        ids, owner, first = self._check_block(emb, ids, owner)
        if (lexical is not None) != getattr(self, "_has_lexical", False) or (token_vecs is not None) != getattr(self, "_has_tokvec", False):
            raise ValueError("insert_rows: the block must bring the lexical postings / token vectors iff the shard holds them")
        if owner == self.rank:
            got = self.engine.index_insert(emb, ids=ids, tenants=tenants, temporal=temporal)
            assert got == first, (got, first)
            if isinstance(lexical, dict):
                self.engine.sparse_append(lexical["indptr"], lexical["doc"], lexical["weight"], lexical["n_docs"], lexical["n_terms_total"])
            elif lexical is not None:
                doc_ptr, terms, weights, n_terms_total = lexical
                self.engine.sparse_append_dev(doc_ptr, terms, weights, n_terms_total)
            if token_vecs is not None:
                self.engine.tokvec_append(token_vecs, token_off)
        self._block_done(ids, owner)
        return owner, first

    def _m3_buffers(self, Q, pool, slots, k, device):
        key = ("m3", Q, pool, slots, k, str(device))
        if key not in self._bufs:
            i64, f64 = torch.int64, torch.float64
            new = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
            send = new((4, Q, pool), i64)
            self._bufs[key] = dict(
                send=send, send_sc=(send[1].view(f64), send[3].view(f64)),      # dense ids | cosine bits | sparse ids | raw sparse bits
                recv=new((self.world, 4, Q, pool), i64), lists=new((2, Q, pool), i64), scores=new((2, Q, pool), f64),
                cand=new((Q, slots), i64), part=new((4, Q, slots), i64), recv2=new((self.world, 4, Q, slots), i64),
                ids=new((Q, k), i64), sc=new((Q, k), f64), comp=new((Q, k, 3), f64))
        return self._bufs[key]

    @staticmethod
    def _slots(pool, mode):
        return 2 * int(pool) if int(mode) == 2 else int(pool)

    def local_lists(self, q_emb, term_ptr, terms, weights, pool, k, mode=2, tenant=-1):
        """This rank's half of the first exchange: [4, Q, pool] int64 = dense ids | cosine bits | sparse ids | raw sparse score
        bits. mode 0 runs no sparse search: its candidates are the dense list and the sparse planes are never read."""
        b = self._m3_buffers(q_emb.shape[0], pool, self._slots(pool, mode), k, q_emb.device)
        send = b["send"]
        self.engine.dense_topk_dev(q_emb, pool, send[0], None, b["send_sc"][0], tenant=tenant)
        if int(mode) != 0:
            self.engine.sparse_topk_dev(term_ptr, terms, weights, pool, send[2], None, b["send_sc"][1], tenant=tenant)
        return send

    def candidates_gathered(self, recv, k, mode=2, rrf_k=60):
        """recv [world, 4, Q, pool]: every rank's local_lists() -> the global candidate ids [Q, slots] (the same on every rank)."""
        _, _, Q, pool = recv.shape
        b = self._m3_buffers(Q, pool, self._slots(pool, mode), k, recv.device)
        self.engine.m3_candidates_gathered_dev(recv, b["lists"], b["scores"], b["cand"], mode=mode, rrf_k=rrf_k)
        return b["cand"]

    def score_local(self, cand, q_emb, term_ptr, terms, weights, q_vecs, q_off, pool, k, w=(0.4, 0.2, 0.4)):
        """This rank's half of the second exchange: [4, Q, slots] int64 = owned flag | dense | sparse | colbert bits."""
        Q, slots = cand.shape
        b = self._m3_buffers(Q, pool, slots, k, cand.device)
        kw = {}
        if float(w[1]) > 0:
            kw.update(term_ptr=term_ptr, terms=terms, weights=weights)
        if float(w[2]) > 0:
            kw.update(q_vecs=q_vecs, q_off=q_off)
        self.engine.m3_score_ids_dev(cand, b["part"], q_emb=q_emb, w=w, **kw)
        return b["part"]

    def combine_gathered(self, cand, recv2, pool, k, w=(0.4, 0.2, 0.4)):
        """cand [Q, slots] and recv2 [world, 4, Q, slots]: every rank's score_local() -> dict(ids, scores, components, candidates)."""
        Q, slots = cand.shape
        b = self._m3_buffers(Q, pool, slots, k, cand.device)
        self.engine.m3_combine_gathered_dev(cand, recv2, b["ids"], b["sc"], b["comp"], w=w)
        return dict(ids=b["ids"], scores=b["sc"], components=b["comp"], candidates=cand)

    def search_m3(self, q_emb, term_ptr, terms, weights, q_vecs, q_off, pool, k, mode=2, w=(0.4, 0.2, 0.4), rrf_k=60, tenant=-1):
        """Replicated CUDA tensors: q_emb [Q, dim] float32, the query CSR term_ptr [Q + 1] / terms int32 / weights float32, q_vecs
        [rows, tok_dim] float32 / q_off [Q + 1] int64; tenant an int or one number per query. Returns dict(ids [Q, k] int64,
        scores [Q, k] float64, components [Q, k, 3] float64 = (dense, sparse, colbert), candidates [Q, slots] int64) - the
        outputs of retrieve_m3_dev on the unsharded index, identical on every rank. world == 1 runs the same path without the
        gathers."""
        Q = q_emb.shape[0]
        b = self._m3_buffers(Q, pool, self._slots(pool, mode), k, q_emb.device)
        send = self.local_lists(q_emb, term_ptr, terms, weights, pool, k, mode=mode, tenant=tenant)
        if self.world == 1:
            recv = send.unsqueeze(0)
        else:
            recv = b["recv"]
            _gather(recv, send, self.group, self.engine)
        cand = self.candidates_gathered(recv, k, mode=mode, rrf_k=rrf_k)
        part = self.score_local(cand, q_emb, term_ptr, terms, weights, q_vecs, q_off, pool, k, w=w)
        if self.world == 1:
            recv2 = part.unsqueeze(0)
        else:
            recv2 = b["recv2"]
            _gather(recv2, part, self.group, self.engine)
        return self.combine_gathered(cand, recv2, pool, k, w=w)

    def search_late_interaction(self, q_emb, q_vecs, q_off, pool, k, term_ptr=None, terms=None, weights=None, rrf_k=60, tenant=-1):
        """The same protocol with weights (0, 0, 1) and mode 0 (term_ptr None) or 1: the score is (1 * c + 0) + 0 over (0 + 0) + 1 =
        c exactly, so ids and score bits are those of retrieve_maxsim_dev on the unsharded index. Returns search_m3's dict."""
        return self.search_m3(q_emb, term_ptr, terms, weights, q_vecs, q_off, pool, k, mode=0 if term_ptr is None else 1, w=(0.0, 0.0, 1.0),
                              rrf_k=rrf_k, tenant=tenant)

    def local_maxsim(self, q_vecs, q_off, k, tenant=-1):
        """This rank's half of search_maxsim: [2, Q, k] int64 = the ids | float64 score bits of the local exhaustive MaxSim search
        (RagEngine.tokvec_search_dev at pool = k)."""
        if not hasattr(self, "_explicit"):
            raise ValueError("search_maxsim: load_shard first (ids must be one id >= 0 per row, strictly ascending on the shard)")
        send, _, _, _, send_ids, send_sc, _ = self._buffers(q_off.shape[0] - 1, k, q_vecs.device)
        ids, sc, _ = self.engine.tokvec_search_dev(q_vecs, q_off, k, pool=k, tenant=tenant)
        send_ids.copy_(ids)
        send_sc.copy_(sc)
        return send

    def merge_maxsim(self, recv):
        """recv [world, 2, Q, k]: every rank's local_maxsim() -> (ids [Q, k] int64, scores [Q, k] float64)."""
        _, _, Q, k = recv.shape
        _, _, out_ids, out_scores, _, _, _ = self._buffers(Q, k, recv.device)
        self.engine.merge_topk_dev(recv, recv.view(torch.float64)[:, 1], out_ids, out_scores, n_lists=self.world, list_stride=2 * Q * k)
        return out_ids, out_scores

    def search_maxsim(self, q_vecs, q_off, k, tenant=-1):
        """The exhaustive MaxSim search over row shards: the local search at k, one gather, rag_merge_topk_dev. A pair's score is a
        function of its own rows and needs no global statistic, so the merged list is the unsharded one - score desc, lower id
        first on ties - wherever id order is row order: implicit ids, or explicit ids ascending with the rows, which is all that
        load_shard and insert_rows accept (ValueError otherwise). Returns (ids [Q, k] int64, scores [Q, k] float64), identical
        on every rank."""
        send = self.local_maxsim(q_vecs, q_off, k, tenant=tenant)
        if self.world == 1:
            return send[0], send[1].view(torch.float64)
        recv = self._buffers(q_off.shape[0] - 1, k, q_vecs.device)[1]
        _gather(recv, send, self.group, self.engine)
        return self.merge_maxsim(recv)

    def search_lexical(self, term_ptr, terms, weights, k, tenant=-1):
        """The learned-sparse top-k alone: local rag_sparse_topk_dev, one gather, rag_merge_topk_dev (raw scores need no global
        statistic). Returns (ids [Q, k] int64, scores [Q, k] float64), score desc, lower id first on ties."""
        Q = term_ptr.shape[0] - 1
        send, recv, out_ids, out_scores, send_ids, send_sc, recv_sc = self._buffers(Q, k, term_ptr.device)
        self.engine.sparse_topk_dev(term_ptr, terms, weights, k, send_ids, None, send_sc, tenant=tenant)
        if self.world == 1:
            return send_ids, send_sc
        _gather(recv, send, self.group, self.engine)
        self.engine.merge_topk_dev(recv, recv_sc, out_ids, out_scores, n_lists=self.world, list_stride=2 * Q * k)
        return out_ids, out_scores


class ShardedReranker:
    """Cross-encoder scoring of P independent (query, passage) pairs split evenly over the ranks; every rank has the
    model loaded (rag_ce_load_host) and receives all P logits. One all_gather of P/world float32 per rank."""

    def __init__(self, engine, rank=None, world=None, group=None):
        self.engine = engine
        self.group = group
        self.world = world if world is not None else (dist.get_world_size(group) if dist.is_initialized() else 1)
        self.rank = rank if rank is not None else (dist.get_rank(group) if dist.is_initialized() else 0)

    def score(self, input_ids, token_type_ids, lens):
        """int32 tensors [P, L], [P, L], [P] replicated on every rank -> float32 logits [P] on every rank."""
        P = input_ids.shape[0]
        per = (P + self.world - 1) // self.world                    # equal slices (the last one may be short)
        lo, hi = min(P, self.rank * per), min(P, (self.rank + 1) * per)
        mine = torch.zeros((per,), dtype=torch.float32, device=input_ids.device)
        if hi > lo:
            self.engine.ce_score_dev(input_ids[lo:hi].contiguous(), token_type_ids[lo:hi].contiguous(),
                                     lens[lo:hi].contiguous(), mine[: hi - lo])
        if self.world == 1:
            return mine[:P]
        out = torch.empty((self.world, per), dtype=torch.float32, device=input_ids.device)
        _gather(out, mine, self.group, self.engine)
        return out.reshape(-1)[:P]


class ShardedPipeline:
    """BASELINE.json configs[4]: row-sharded hybrid retrieval + cross-encoder rerank. Every rank holds its row shard
    (embeddings + doc-partitioned postings), the cross-encoder weights and a REPLICATED passage token store (it fits:
    100M x 256 tokens x 2 B = 51 GB of 288 GB; loaded with ids starting at token_id_base). Three small collectives per
    batch: the candidate lists (ShardedHybridIndex), nothing for the pair assembly (every rank builds all pairs from the
    merged global ids), the logits (ShardedReranker). Every rank ends with the same top-k."""

    def __init__(self, engine, rank=None, world=None, group=None, token_id_base=0):
        self.engine = engine
        self.index = ShardedHybridIndex(engine, rank=rank, world=world, group=group)
        self.reranker = ShardedReranker(engine, rank=rank, world=world, group=group)
        self.token_id_base = token_id_base
        self._bufs = {}

    def retrieve_rerank(self, queries, term_ptr, terms, q_tok, q_len, pool, k, L_pair=512, rrf_k=60, cls_id=101, sep_id=102, tenant=-1):
        """Returns (ids [Q,k] int64, scores [Q,k] float64 = sigmoid(logit), logits [Q,k] float32, candidates [Q,pool])."""
        Q, dev = queries.shape[0], queries.device
        cand = self.index.search_hybrid(queries, term_ptr, terms, pool, pool, rrf_k=rrf_k, tenant=tenant)["keys"]
        key = (Q, pool, k, L_pair, str(dev))
        if key not in self._bufs:
            P = Q * pool
            self._bufs[key] = (torch.empty((P, L_pair), dtype=torch.int32, device=dev), torch.empty((P, L_pair), dtype=torch.int32, device=dev),
                               torch.empty((P,), dtype=torch.int32, device=dev), torch.empty((Q, k), dtype=torch.int64, device=dev),
                               torch.empty((Q, k), dtype=torch.float64, device=dev), torch.empty((Q, k), dtype=torch.float32, device=dev))
        pid, ptt, plen, ids, sc, lg = self._bufs[key]
        self.engine.ce_build_pairs_dev(q_tok, q_len, cand, pid, ptt, plen, token_id_base=self.token_id_base, cls_id=cls_id, sep_id=sep_id)
        logits = self.reranker.score(pid, ptt, plen).contiguous()
        self.engine.rerank_topk_dev(logits, cand, ids, sc, lg)
        return ids, sc, lg, cand
