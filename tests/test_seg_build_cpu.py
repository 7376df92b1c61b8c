"""CPU: ii2_seg_build / PutBatch are wired through every layer - header, binding, Makefile, host mirror and its Python
face - and the sort's source keeps to its rule that no workgroup waits for another."""
import ctypes as C
import os
import re

from inverted_index_2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "inverted_index_2_amd", "csrc")


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "ii2.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(ii2_[a-z0-9_]+)\s*\(", text))


def test_seg_build_is_declared_and_bound():
    assert "ii2_seg_build" in _header_symbols()
    assert "ii2_seg_build" in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES["ii2_seg_build"]
    assert res is C.c_int and len(args) == 8
    # the stats structure as the header lays it out: three u64 and one u32 (padded to 32 bytes)
    assert [f[0] for f in _lib.BuildStats._fields_] == ["n_pairs", "n_postings", "n_nonempty", "n_passes"]
    assert C.sizeof(_lib.BuildStats) == 32


def test_seg_build_object_is_in_the_makefile():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(line for line in mk.splitlines() if line.startswith("OBJS"))
    assert "build/seg_build.o" in objs.split()


def test_host_library_exports_put_batch():
    from inverted_index_2_amd import host
    if not os.path.exists(host.HOST_LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    C.CDLL(_lib.LIB_PATH)        # dependency first
    assert hasattr(C.CDLL(host.HOST_LIB_PATH), "ii2h_put_batch")


def test_python_face_has_put_batch_and_build_segment():
    from inverted_index_2_amd import Context, host
    assert callable(getattr(host.Shard, "put_batch", None))
    assert callable(getattr(host.InvertedIndex, "put_batch", None))
    assert callable(getattr(Context, "build_segment", None))


def test_sort_has_no_inter_workgroup_waits():
    src = open(os.path.join(CSRC, "seg_build.hip")).read()
    assert "lookback.h" not in src and "ii2_lookback_launch" not in src
    # the three sort kernels, the dedupe pass and the offsets are all there
    for k in ("k_sb_hist", "k_sb_scatter", "k_sb_heads", "k_sb_offsets"):
        assert k in src, k
