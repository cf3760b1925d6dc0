"""Exact tree search between free-form point lists (dl_nn_list_*): what can be checked without a GPU -- the four entry points are
declared, exported and bound, the sizes of the caller-owned buffers are the figures include/delora_hip.h states, and bad arguments
are refused by name before anything is launched."""
import ctypes
import os
import re

import pytest

from tests.conftest import ROOT

ENTRY_POINTS = ("dl_nn_list_tree_bytes", "dl_nn_list_query_workspace_bytes", "dl_nn_list_build", "dl_nn_list_query")
MAX_POINTS = 1 << 30


def _lib_loaded():
    from delora_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def tree_bytes(Mt):
    """The header's formula: 8192 + 40 P + 32 nodes + 1024 ceil(Mt / 2048)."""
    P = (Mt + 63) // 64 * 64
    nodes, n = 0, P // 64
    while n > 0:
        nodes += n
        if n <= 64:
            break
        n = (n + 63) // 64
    return 8192 + 40 * P + 32 * nodes + 1024 * ((Mt + 2047) // 2048)


def query_bytes(Ms):
    """The header's formula: 24 Q + 1024 ceil(Ms / 2048)."""
    return 24 * ((Ms + 63) // 64 * 64) + 1024 * ((Ms + 2047) // 2048)


def test_entry_points_are_declared_exported_and_bound():
    from delora_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "delora_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dl_[a-z0-9_]+)\s*\(", text))
    lib = _lib_loaded()
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["dl_nn_list_tree_bytes"][0] is ctypes.c_size_t
    assert _lib.SIGNATURES["dl_nn_list_query_workspace_bytes"][0] is ctypes.c_size_t
    assert len(_lib.SIGNATURES["dl_nn_list_build"][1]) == 5 and len(_lib.SIGNATURES["dl_nn_list_query"][1]) == 10
    assert lib.dl_abi_version() == 10 == _lib.ABI_VERSION
    assert "#define DL_ABI_VERSION 10 " in open(os.path.join(ROOT, "include", "delora_hip.h")).read()


COUNTS = (0, 1, 2, 63, 64, 65, 1000, 2048, 2049, 4096, 4097, 32768, 70001, 131072, 262144, 262145, 1 << 24, (1 << 24) + 1, MAX_POINTS)


def test_buffer_sizes_are_the_documented_figures():
    lib = _lib_loaded()
    for fn, formula, per_point in ((lib.dl_nn_list_tree_bytes, tree_bytes, 16), (lib.dl_nn_list_query_workspace_bytes, query_bytes, 0)):
        assert fn(-1) == 0 and fn(-(1 << 31)) == 0                   # a negative count has no size
        assert fn(MAX_POINTS + 1) == 0 and fn((1 << 31) - 1) == 0      # nor has one beyond the 32-bit guard
        last = -1
        for m in COUNTS:
            got = fn(m)
            assert got == formula(m), (fn, m, got, formula(m))
            assert got >= per_point * m and got >= last and got % 16 == 0, (m, got)
            last = got
    assert lib.dl_nn_list_tree_bytes(0) == 8192 and lib.dl_nn_list_query_workspace_bytes(0) == 0
    # per point: 40 B of records, keys and indices, about one more of boxes and digit counts -- a workspace that grows shows here
    assert 40.0 <= (lib.dl_nn_list_tree_bytes(262144) - 8192) / 262144 <= 41.1
    assert 24.0 <= lib.dl_nn_list_query_workspace_bytes(262144) / 262144 <= 24.6
    # monotone between the listed counts as well
    sizes = [lib.dl_nn_list_tree_bytes(m) for m in range(0, 9000)]
    assert sizes == sorted(sizes)
    sizes = [lib.dl_nn_list_query_workspace_bytes(m) for m in range(0, 9000)]
    assert sizes == sorted(sizes)


def test_bad_arguments_are_refused_by_name():
    lib = _lib_loaded()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)           # an aligned host address: never dereferenced on these paths

    def refused(rc, name, word=None):
        msg = lib.dl_last_error()
        assert rc < 0 and name.encode() in msg, (rc, msg)
        if word:
            assert word.encode() in msg, msg

    refused(lib.dl_nn_list_build(None, 8, 8, p, None), "dl_nn_list_build", "null")
    refused(lib.dl_nn_list_build(p, 8, 8, None, None), "dl_nn_list_build", "null")
    refused(lib.dl_nn_list_build(p, 8, -1, p, None), "dl_nn_list_build", "negative")
    refused(lib.dl_nn_list_build(p, 4, 8, p, None), "dl_nn_list_build", "stride")
    refused(lib.dl_nn_list_build(p, 8, 8, ctypes.c_void_p(p.value + 4), None), "dl_nn_list_build", "aligned")
    refused(lib.dl_nn_list_build(p, 1 << 31, MAX_POINTS + 1, p, None), "dl_nn_list_build")
    for args in ((None, 8, 8, None, 0, 8, p, p, p, None), (p, 8, 8, None, 0, 8, None, p, p, None), (p, 8, 8, None, 0, 8, p, None, p, None),
                 (p, 8, 8, None, 0, 8, p, p, None, None)):
        refused(lib.dl_nn_list_query(*args), "dl_nn_list_query", "null")
    refused(lib.dl_nn_list_query(p, 8, -1, None, 0, 8, p, p, p, None), "dl_nn_list_query", "negative")
    refused(lib.dl_nn_list_query(p, 8, 8, None, 0, -1, p, p, p, None), "dl_nn_list_query", "negative")
    refused(lib.dl_nn_list_query(p, 4, 8, None, 0, 8, p, p, p, None), "dl_nn_list_query", "stride")
    refused(lib.dl_nn_list_query(p, 8, 8, None, 0, 8, p, p, ctypes.c_void_p(p.value + 8), None), "dl_nn_list_query", "aligned")
    # an empty query list is not an error, whatever else is passed
    assert lib.dl_nn_list_query(None, 0, 0, None, 0, 8, None, None, None, None) == 0


def test_cpu_tensors_are_rejected_not_emulated():
    import torch
    from delora_amd import _lib, geometry
    _lib_loaded()
    with pytest.raises(_lib.DeloraHipError):
        geometry.PointTree(torch.zeros((3, 8)))
