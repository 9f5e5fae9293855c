"""Every grow-only device buffer of a handle is grown with work queued by some test and used again after a change of shape or
state by some test - or has a stated reason for needing neither.

The sources (optimized-rag_amd/csrc/*.hip and common.h) are scanned for the places where a call carves such a buffer by its own
shape: `<buffer>.reserve(h, ...)` (common.h dev_buf::reserve: "contents are NOT kept"), a `ws_carve` over a buffer, a call of
`pipe_ws_carve`, the `need > <buffer>.size()` form of linear_carve, `stage_reserve`, the two workspaces that are renewed as a
whole (`Q <= h->ws_q` in dense.hip, `ws_renew` in cross_encoder.hip), and every `<buffer>.reset()` of a buffer found so (a reset
decides which test can re-use the buffer at all: live.hip frees lin_ws on every live write). A site is (buffer, the function it
stands in). TABLE maps
each to two cases, named as `file::test` or `file::test[parameter]`:
  grown   the buffer is re-allocated by a larger call while earlier work of the handle is still queued on the stream
  reused  the buffer is carved again by another shape, or after the index changed, and the result compared with a fresh handle
or to `exempt: <reason>`. A new site fails here until it has both; a case that no test file defines fails too. Runs without a GPU."""
import os
import re

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "optimized-rag_amd", "csrc")

CALLS = "tests/test_call_history_gpu.py::test_small_large_small_on_one_handle"
MIXED = "tests/test_call_history_gpu.py::test_one_pipeline_workspace_under_four_composites"
STATE = "tests/test_state_history_gpu.py::test_the_batch_after_the_writes_is_that_of_a_fresh_handle"
FIRST = "tests/test_stream_order_gpu.py::"
SLACK = "tests/test_cross_encoder_shapes_gpu.py::test_stale_nan_rows_of_a_larger_call_do_not_reach_a_later_call"
FIXED = "exempt: a flag or counter block of a fixed size, allocated once"
HOST = (FIRST + "test_small_device_batch_then_large_host_batch", FIRST + "test_host_call_behind_a_queued_device_call")
HOST_WHY = "the staging arena of the synchronous *_host entries (they wait for the device first); grown and reused by: "

TABLE = {
    ("pipe_ws", "retrieve_rerank_dev"): (FIRST + "test_pipeline_workspace_grows_with_work_queued", MIXED),
    ("pipe_ws", "retrieve_maxsim_dev"): (CALLS + "[retrieve_maxsim_dev]", MIXED),
    ("pipe_ws", "m3_score_rows_dev"): (CALLS + "[m3_score_rows_dev]", CALLS + "[m3_score_rows_dev]"),
    ("pipe_ws", "retrieve_m3_dev"): (CALLS + "[retrieve_m3_dev-count]", CALLS + "[retrieve_m3_dev-mode_1_2_1]"),
    ("pipe_ws", "m3_candidates_gathered_dev"): (CALLS + "[m3_shard_chain-implicit_ids]", CALLS + "[m3_shard_chain-explicit_ids]"),
    ("pipe_ws", "m3_score_ids_dev"): (CALLS + "[m3_shard_chain-explicit_ids]", CALLS + "[m3_shard_chain-implicit_ids]"),
    ("pipe_ws", "search_m3_tokens_dev"): (CALLS + "[search_m3_tokens_dev-count]", CALLS + "[search_m3_tokens_dev-mode_0_2_0]"),
    ("pipe_ws", "pipe_ws_carve"): (CALLS + "[retrieve_m3_dev-pool]", MIXED),
    ("ix->ws", "bm25_dev_ws"): (CALLS + "[sparse_topk_dev]", CALLS + "[sparse_topk_tenants_dev]"),
    ("lin_ws", "linear_carve"): ("exempt: lin_ws is sized by the row count, which only a host write changes, and a host write waits for the device; "
                                 "a live write frees it (the site below), so after an insert it is allocated anew, not grown",
                                 STATE + "[shrink_by_replacement]"),
    ("lin_ws", "live_rows_changed"): ("exempt: the reset of lin_ws by every live write that changes the row count (compactions, inserts): the next "
                                      "linear call allocates and zero-fills it, in " + STATE + "[grow_inside_a_reservation]",
                                      "exempt: nothing is re-used behind it: " + STATE + "[shrink_by_compaction] runs on a new lin_ws"),
    ("tv_ws", "tokvec_score_slots"): (CALLS + "[tokvec_rerank_dev-fp16]", CALLS + "[tokvec_rerank_dev-mxfp8]"),
    ("side_scores", "hybrid_legs"): ("exempt: reserved at RAG_FORK_MAX_Q x RAG_MAX_K, the most a forked leg can ask: it never grows",
                                     CALLS + "[hybrid_sparse_rrf_dev]"),
    ("qten", "stage_query_tenants"): (CALLS + "[hybrid_rrf_tenants_dev]", CALLS + "[hybrid_rrf_tenants_dev]"),
    ("union_tiles", "search_tiles"): ("exempt: reserved for every tile of the index and at least 1024: it grows only past 262,144 rows, after a host write",
                                      CALLS + "[hybrid_linear_tenants_dev]"),
    ("scan_scores", "exact_scan_rounds"): (CALLS + "[dense_topk_tenants_dev-exact_scan]", CALLS + "[dense_topk_tenants_dev-exact_scan]"),
    ("ws", "ensure_workspace"): (FIRST + "test_dense_workspace_grows_with_work_queued", CALLS + "[hybrid_linear_tenants_dev]"),
    ("stats", "ensure_workspace"): (FIXED, FIXED),
    ("tv_bad", "tokvec_reserve"): (FIXED, FIXED),
    ("tok_bad", "tokens_reserve"): (FIXED, FIXED),
    ("ce_ws", "ce_ensure_ws"): (FIRST + "test_cross_encoder_workspace_grows_with_work_queued", SLACK),
    ("ce_ws", "mx_ensure_ws"): (FIRST + "test_cross_encoder_workspace_grows_with_work_queued", SLACK),
}
# the callers of stage_reserve and the keyword host search's ws_carve over h->stage: one arena, one pair of cases (HOST)
STAGE = {"bm25_run", "chunk_chain_host", "dense_topk_host_entry", "linear_fuse_topk_host", "mmr_select_host", "pairwise_cosine_host_t",
         "rag_index_rows_of_ids_host", "rrf_fuse_host", "stage_id_set", "tokens_load_host"}


def functions(text):
    """(line number, name) of every function definition that starts in column 0"""
    out = []
    for i, line in enumerate(text.split("\n")):
        m = re.match(r"^[A-Za-z_][^;#]*?\b(\w+)\($|^[A-Za-z_][^;#]*?\b(\w+)\([^;]*$|^[A-Za-z_][^;#(]*?\b(\w+)\([^;{]*\)\s*\{.*\}\s*$", line)
        if m and not line.startswith(("return", "if", "else", "for", "while", "struct", "using", "typedef")):
            out.append((i, m.group(1) or m.group(2) or m.group(3)))
    return out


def sites():
    found = set()
    names = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip") or f == "common.h")
    for name in names:
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        defs = functions(text)

        def where(i):
            inside = [n for at, n in defs if at <= i]
            return inside[-1] if inside else "?"

        for i, line in enumerate(text.split("\n")):
            code = line.split("//")[0]
            for m in re.finditer(r"([\w>.-]+)\.reserve\(h,", code):
                found.add((m.group(1).replace("h->", ""), where(i)))
            if "pipe_ws_carve(" in code and not re.match(r"^static int pipe_ws_carve", code):
                found.add(("pipe_ws", where(i)))
            if re.search(r"\bws_carve\b", code):
                for m in re.finditer(r"\b\w+\{([\w>.-]+)\}", code):
                    if m.group(1) != "nullptr":
                        found.add((m.group(1).replace("h->", ""), where(i)))
            for m in re.finditer(r"need > h->(\w+)\.size\(\)", code):
                found.add((m.group(1), where(i)))
            if re.search(r"\bstage_reserve\(h", code) and not code.startswith("static inline int stage_reserve"):
                found.add(("stage", where(i)))
            if re.search(r"<= h->ws_q\b", code):
                found.add(("ws", where(i)))
            if re.search(r"\bws_renew\(h", code) and not code.startswith("static int ws_renew"):
                found.add(("ce_ws", where(i)))
    grow_only = {b for b, _ in found}
    for name in names:                                      # second pass: where one of these buffers is dropped
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        defs = functions(text)
        for i, line in enumerate(text.split("\n")):
            for m in re.finditer(r"([\w>.-]+)\.reset\(\)", line.split("//")[0]):
                buf = m.group(1).replace("h->", "")
                if buf in grow_only:
                    inside = [n for at, n in defs if at <= i]
                    found.add((buf, inside[-1] if inside else "?"))
    return found


def test_the_scan_finds_the_sites_this_table_was_written_for():
    found = sites()
    buffers = {b for b, _ in found}
    assert {"pipe_ws", "ix->ws", "lin_ws", "tv_ws", "side_scores", "qten", "scan_scores", "union_tiles", "stage", "ws", "ce_ws"} <= buffers, sorted(buffers)
    assert sum(1 for b, _ in found if b == "pipe_ws") >= 8
    assert ("lin_ws", "live_rows_changed") in found


def test_every_site_has_a_growth_case_and_a_reuse_case_or_a_reason():
    found = sites()
    missing = sorted(s for s in found if s not in TABLE and s[0] != "stage")
    assert not missing, f"grow-only sites without a line in TABLE: {missing}"
    gone = sorted(s for s in TABLE if s not in found)
    assert not gone, f"TABLE names sites the sources no longer hold: {gone}"
    stage = {fn for b, fn in found if b == "stage"}
    assert stage == STAGE, f"{HOST_WHY}{HOST}; the sites changed: {sorted(stage ^ STAGE)}"


def defined(case):
    """does `file::test` or `file::test[parameter]` name a test function of that file and a parameter the file spells out?"""
    m = re.match(r"^(tests/\w+\.py)::(\w+)(?:\[(.+)\])?$", case)
    if not m:
        return False
    with open(os.path.join(ROOT, m.group(1))) as f:
        text = f.read()
    return re.search(r"^def " + m.group(2) + r"\(", text, re.M) is not None and (m.group(3) is None or f'"{m.group(3)}"' in text)


def test_every_named_case_exists_and_every_exemption_gives_a_reason():
    for site, pair in TABLE.items():
        assert len(pair) == 2
        for what in pair:
            if what.startswith("exempt: "):
                assert len(what.split()) >= 6, f"{site}: an exemption is a sentence"
            else:
                assert defined(what), f"{site}: no such case: {what}"
    assert all(defined(c) for c in HOST)
