"""CPU-only: the host side of sequences past 512 tokens - rag_ce_length_class (the length-class table per head width and its limits,
no GPU call) and cross_encoder.seq_limit (the limit the Python classes cut max_length at). Before the long length classes existed
neither the symbol nor the function did."""
import ctypes as C

import pytest

import __graft_entry__ as G

RAG_ERR_ARG = -1
CLASSES_TO_512 = [32, 64, 96, 128, 192, 256, 384, 512]          # the table every model had before the long classes
LONG_CLASSES = [768, 1024, 1536, 2048, 3072, 4096, 6144, 8192]


@pytest.fixture(scope="module")
def lib():
    G.build()
    import optimized_rag_amd
    return optimized_rag_amd.load_library()


def _cls(lib, head_dim, seq_len):
    out = C.c_int(-7)
    rc = lib.rag_ce_length_class(head_dim, seq_len, C.byref(out))
    return (rc, out.value)


def test_length_class_check_points(lib):
    for seq_len, want in ((512, 512), (513, 768), (768, 768), (769, 1024), (1025, 1536), (6145, 8192), (8192, 8192)):
        assert _cls(lib, 64, seq_len) == (0, want), seq_len
    assert _cls(lib, 64, 8193) == (RAG_ERR_ARG, -7)
    assert _cls(lib, 32, 512) == (0, 512)
    assert _cls(lib, 32, 513) == (RAG_ERR_ARG, -7)
    for seq_len in (1, 64, 512, 513, 8192):
        assert _cls(lib, 48, seq_len) == (RAG_ERR_ARG, -7)
    for head_dim in (32, 64):
        assert _cls(lib, head_dim, 0)[0] == RAG_ERR_ARG and _cls(lib, head_dim, -5)[0] == RAG_ERR_ARG
    assert lib.rag_ce_length_class(64, 100, None) == RAG_ERR_ARG


def test_every_seq_len_gets_the_smallest_class_that_holds_it(lib):
    """Up to 512 both head widths return the class of the table every model had before; above, 64-wide heads return the smallest long
    class, at every seq_len up to 8192."""
    for seq_len in range(1, 513):
        want = next(c for c in CLASSES_TO_512 if c >= seq_len)
        assert _cls(lib, 32, seq_len) == (0, want) and _cls(lib, 64, seq_len) == (0, want), seq_len
    for seq_len in range(513, 8193):
        assert _cls(lib, 64, seq_len) == (0, next(c for c in LONG_CLASSES if c >= seq_len)), seq_len


def test_seq_limit_of_a_config():
    from optimized_rag_amd.cross_encoder import MINILM_L6_CONFIG, seq_limit
    shape = lambda hidden, heads, max_pos: dict(vocab_size=1000, hidden=hidden, layers=2, heads=heads, ffn=4 * hidden, max_pos=max_pos)
    assert seq_limit(MINILM_L6_CONFIG) == 512                     # 384 / 12: 32-wide heads
    assert seq_limit(shape(768, 12, 512)) == 512                  # BERT-base: its position table
    assert seq_limit(shape(1024, 16, 8192)) == 8192               # XLM-R-large, bge-m3's table (8194 rows less the 2 reserved)
    assert seq_limit(shape(1024, 16, 3000)) == 3000
    assert seq_limit(shape(1024, 16, 20000)) == 8192
    assert seq_limit(shape(128, 4, 8192)) == 512                  # 32-wide heads stay at 512 whatever the table holds


def test_the_engine_wrappers_exist():
    from optimized_rag_amd import RagEngine
    assert callable(RagEngine.model_seq_limit) and callable(RagEngine.ce_length_class)
