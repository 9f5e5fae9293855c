"""Every device-pointer entry of include/rag_hip.h has a stream-order test, or a stated reason for having none.

The declarations `rag_*_dev(` of the header are held against the cases of tests/test_stream_order_gpu.py (case name up to the
first "-" = the entry without its `rag_` prefix) and of tests/test_stream_order_resident_gpu.py (its ENTRIES table, which its
late-producer test checks against the entries the Python wrapper really called). A new `*_dev` entry fails here until it gets a
case or a line in EXEMPT; a case that names an entry the header does not declare fails too. Runs without a GPU: both modules
import torch lazily."""
import os
import re

import test_stream_order_gpu as A
import test_stream_order_resident_gpu as R

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rag_hip.h")
EXEMPT = {
    "rag_comm_allgather_dev": "needs a communicator of several ranks; tests/test_sharded_two_ranks_gpu.py and the other two-rank tests run it",
}


def declared():
    with open(HEADER) as f:
        return set(re.findall(r"\b(rag_\w+_dev)\(", f.read()))


def covered():
    first = {"rag_" + name.split("-")[0] for name in A.CASES}
    second = {entry for name in R.CASES for entry in R.ENTRIES[name]}
    return first, second


def test_the_header_declares_the_entries_this_table_was_written_for():
    names = declared()
    assert len(names) >= 50 and {"rag_dense_topk_dev", "rag_search_m3_tokens_tenants_dev", "rag_index_rows_of_ids_dev"} <= names


def test_every_device_pointer_entry_has_a_stream_order_case_or_a_reason():
    first, second = covered()
    missing = sorted(declared() - first - second - set(EXEMPT))
    assert not missing, f"no case in tests/test_stream_order_gpu.py or tests/test_stream_order_resident_gpu.py, and no line in EXEMPT: {missing}"
    assert all(isinstance(why, str) and len(why.split()) >= 4 for why in EXEMPT.values())


def test_no_case_names_an_entry_the_header_does_not_declare():
    first, second = covered()
    unknown = sorted((first | second | set(EXEMPT)) - declared())
    assert not unknown, unknown
    both = sorted(set(EXEMPT) & (first | second))
    assert not both, f"exempt and covered at once: {both}"


def test_every_case_of_the_resident_file_lists_its_entries():
    assert set(R.ENTRIES) == set(R.CASES)
    assert all(R.ENTRIES[name] for name in R.CASES)
    assert set(R.STATELESS) == {name for name, (_, asynchronous) in R.CASES.items() if asynchronous}
