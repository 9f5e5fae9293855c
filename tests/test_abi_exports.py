"""CPU-only: the C-ABI library builds for gfx950, loads, and exports every symbol include/rag_hip.h declares.
No compute calls (there is no GPU here)."""
import ctypes
import os
import re

import pytest

import __graft_entry__ as G
import guard_tools


@pytest.fixture(scope="module")
def lib():
    G.build()
    import optimized_rag_amd
    return optimized_rag_amd.load_library()


def test_header_symbols_all_exported(lib):
    from optimized_rag_amd import _lib
    hdr = open(os.path.join(G.ROOT, "include", "rag_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(rag_[a-z0-9_]+)\s*\(", hdr)))
    assert declared, "no declarations parsed"
    assert declared == _lib.exported_symbols(), "ctypes signature table and header disagree"
    for name in declared:
        assert hasattr(lib, name), f"{name} not exported by librag_hip.so"


def test_version_and_null_handle(lib):
    assert lib.rag_version() >= 100
    assert lib.rag_destroy(None) != 0
    assert lib.rag_last_error(None) == b"null handle"


def test_no_cpu_fallback_without_gpu(lib):
    """Without a GPU, creating an engine must fail loudly rather than fall back to a CPU path."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from optimized_rag_amd import RagEngine, RagError
    with pytest.raises(RagError):
        RagEngine(dim=1536, device=0)


def test_product_never_imports_oracle():
    pkg = os.path.join(G.ROOT, "optimized-rag_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dp, f)).read()
                assert "oracle" not in src.replace("the float64 oracle", "").replace("oracle's", ""), f


def test_bench_reads_the_committed_traffic_profile():
    """bench.py fills roofline.traffic from profiles/r02_g_dense_pmc.json: the file must carry the key it reads (a reshaped
    file once took the default bench line down; bench.py now also tolerates it)."""
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "r02_g_dense_pmc.json")) as f:
        total = json.load(f)["kernels"]["dense_emit_kernel<false>"]["hbm_traffic_bytes_per_launch"]["total"]
    assert 1.0e9 < total < 3.0e9            # ~1.5 GB per launch against 1.025 GB algorithmic


# ---- argument kinds and struct layouts: the header against the hand-typed ctypes table ------------------------------------------
def c_kind(decl):
    """pointer | int | int64 | double | float | size_t of one C parameter or return type (rag_handle_t is a pointer)"""
    decl = decl.strip()
    if "*" in decl or "[" in decl or re.search(r"\brag_handle_t\b", decl):
        return "pointer"
    words = [w for w in re.findall(r"[A-Za-z_]\w*", decl) if w not in ("const", "unsigned", "signed", "struct")]
    for kind, names in (("int64", ("int64_t",)), ("int", ("int", "int32_t")), ("double", ("double",)), ("float", ("float",)),
                        ("size_t", ("size_t",))):
        if words and words[0] in names:
            assert "unsigned" not in decl, decl
            return kind
    raise AssertionError(f"parameter of no known kind: {decl!r}")


def header_prototypes():
    """name -> (parameter kinds in order, return kind) of every prototype of the header (guard_tools parses them)"""
    return {name: ([c_kind(p) for p in params], c_kind(ret)) for name, (params, ret) in guard_tools.header_declarations().items()}


def ctypes_kind(t):
    if t is ctypes.c_void_p or t is ctypes.c_char_p or isinstance(t, type(ctypes.POINTER(ctypes.c_int))):
        return "pointer"
    for kind, types in (("int", (ctypes.c_int, ctypes.c_int32)), ("int64", (ctypes.c_int64,)), ("double", (ctypes.c_double,)),
                        ("float", (ctypes.c_float,)), ("size_t", (ctypes.c_size_t,))):
        if any(t is x for x in types):
            return kind
    raise AssertionError(f"ctypes type of no known kind: {t!r}")


def test_the_parser_tells_the_kinds_apart():
    """the check below is only as good as c_kind: one declaration of every kind, a multi-line one and a commented one"""
    assert c_kind("const int64_t* ids_host") == "pointer" and c_kind("rag_handle_t h") == "pointer" and c_kind("void* stream") == "pointer"
    assert [c_kind(p) for p in ("int k", "int32_t n", "int64_t n_rows", "double lambda", "float lex_b", "size_t nbytes", "const int k")] == \
        ["int", "int", "int64", "double", "float", "size_t", "int"]
    assert ctypes.sizeof(ctypes.c_int) == 4 and ctypes.c_int64 is not ctypes.c_size_t
    protos = header_prototypes()
    assert protos["rag_version"] == ([], "int")
    assert protos["rag_last_error"] == (["pointer"], "pointer")
    assert protos["rag_index_load_dev"] == (["pointer", "pointer", "pointer", "int64", "int64", "pointer"], "int")
    assert protos["rag_comm_allgather_dev"][0][3] == "size_t"
    assert protos["rag_embed_heads_load_host"][0][-1] == "float"


def test_every_signature_has_the_headers_argument_kinds():
    """count, order and kind of every parameter and the return kind: a c_int where the header says int64_t, or a missing trailing
    void* stream, passes every compute test at small values"""
    from optimized_rag_amd import _lib
    protos = header_prototypes()
    assert sorted(protos) == _lib.exported_symbols()
    wrong = {}
    for name, (args, res) in _lib._SIGS.items():
        mine = ([ctypes_kind(a) for a in args], ctypes_kind(res))
        if mine != protos[name]:
            wrong[name] = dict(ctypes=mine, header=protos[name])
    assert not wrong, wrong


STRUCTS = {"rag_dense_stats": "DenseStats", "rag_row_block": "RowBlock", "rag_id_map_info": "IdMapInfo",
           "rag_bm25_segments": "Bm25Segments", "rag_bm25_refresh_info": "Bm25RefreshInfo", "rag_ce_config": "CeConfig"}


def header_struct_fields():
    """struct name -> field names in declaration order (`int32_t a, b;` declares two)"""
    found = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", guard_tools.header_text(), flags=re.S):
        fields = []
        for stmt in body.split(";"):
            if stmt.strip():
                fields += [re.findall(r"[A-Za-z_]\w*", part)[-1] for part in stmt.split(",")]
        found[name] = fields
    return found


def test_struct_mirrors_have_the_compilers_layout(tmp_path):
    """sizeof, and every field's name, offsetof and size as the build's compiler lays the header's structs out for the host,
    against the _fields_ of the ctypes mirrors in declaration order"""
    import subprocess
    from optimized_rag_amd import _lib
    fields = header_struct_fields()
    assert sorted(fields) == sorted(STRUCTS), "a struct of the header has no entry in STRUCTS (or the reverse)"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "rag_hip.h"', 'int main(void) {']
    for s, names in fields.items():
        lines.append(f'    printf("{s} %zu\\n", sizeof({s}));')
        for f in names:
            lines.append(f'    printf("{s}.{f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));')
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")           # the Makefile's compiler; -x c: host only, no device pass
    subprocess.run([hipcc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(G.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        key, *nums = line.split()
        got[key] = tuple(int(n) for n in nums)
    for s, names in fields.items():
        mirror = getattr(_lib, STRUCTS[s])
        assert [n for n, _ in mirror._fields_] == names, s
        assert ctypes.sizeof(mirror) == got[s][0], s
        for n, t in mirror._fields_:
            assert (getattr(mirror, n).offset, ctypes.sizeof(t)) == got[f"{s}.{n}"], f"{s}.{n}"
